"""FP64 MFMA toolkit vs numpy/LAPACK (FP64).  Tolerances: GEMM 1e-12 relative to |A||B|,
Cholesky / inverse 1e-10 relative on well-conditioned SPD matrices.

Two rules for the GEMM tests that mean a particular kernel:
* exact integers: operands with integer entries in -8 .. 8 make every partial sum an integer far below 2^53, so the
  FP64 sum is exact in any order and the result must be `array_equal` to numpy's -- a skipped, repeated or misplaced
  k-tile shows with no tolerance to argue about; the same case then runs on standard normals under the rounded bound
  max |got - ref| / (|A| |B|) < 1e-14 K;
* counters: which of the two tile kernels a shape runs on is the library's decision (a cost rule that may be retuned),
  so a test never restates it: it reads `gemm_launches_128` / `gemm_launches_64` (gss_stat) around its product and
  asserts that the kernel it means is the one that ran."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _gemm(M, N, K, A, sa, B, sb, D, sd, alpha=1.0, beta=0.0, lower=0):
    from gss import _lib
    l = _lib.lib()
    _lib.check(l.gss_dev_gemm(M, N, K, alpha, _lib.ptr(A), sa[0], sa[1], _lib.ptr(B), sb[0], sb[1], beta,
                              _lib.ptr(D), sd[0], sd[1], lower, _lib.current_stream()))


@pytest.mark.parametrize("M,N,K", [(16, 16, 4), (128, 128, 16), (130, 67, 33), (257, 300, 129), (5, 1000, 1000)])
def test_gemm_all_layouts_asymmetric(M, N, K):
    import torch
    rng = np.random.default_rng(M * 7 + N)
    A = rng.normal(size=(M, K))
    B = rng.normal(size=(K, N))
    ref = A @ B
    scale = np.abs(A) @ np.abs(B)
    for a_cm in (False, True):
        for b_cm in (False, True):
            for d_cm in (False, True):
                dA = _t(A.T if a_cm else A)          # column-major image when a_cm
                dB = _t(B.T if b_cm else B)
                dD = torch.zeros((N, M) if d_cm else (M, N), dtype=torch.float64, device="cuda")
                sa = (1, M) if a_cm else (K, 1)
                sb = (1, K) if b_cm else (N, 1)
                sd = (1, M) if d_cm else (N, 1)
                _gemm(M, N, K, dA, sa, dB, sb, dD, sd)
                got = dD.cpu().numpy()
                got = got.T if d_cm else got
                assert np.max(np.abs(got - ref) / scale) < 1e-14 * K


def test_gemm_identity_catches_transposed_output():
    import torch
    n = 64
    B = np.arange(n * n, dtype=np.float64).reshape(n, n)     # asymmetric
    dI, dB = _t(np.eye(n)), _t(B)
    dD = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    _gemm(n, n, n, dI, (n, 1), dB, (n, 1), dD, (n, 1))
    assert np.array_equal(dD.cpu().numpy(), B)


def test_gemm_alpha_beta_and_lower_only():
    import torch
    rng = np.random.default_rng(5)
    n, k = 300, 70
    A = rng.normal(size=(n, k))
    C0 = rng.normal(size=(n, n))
    dA, dC = _t(A.T), _t(C0.T.copy())                          # column-major
    _gemm(n, n, k, dA, (1, n), dA, (n, 1), dC, (1, n), alpha=-1.0, beta=1.0, lower=1)
    got = dC.cpu().numpy().T
    ref = C0 - A @ A.T
    il = np.tril_indices(n)
    assert np.allclose(got[il], ref[il], atol=1e-11)
    # tiles strictly above the diagonal blocks are untouched
    assert np.array_equal(got[:128, 128:], C0[:128, 128:])


# ---------------------------------------------------------------------------------------------
# the 128 x 128 tile kernel and the zero-structure modes, each pinned by the launch counters
# ---------------------------------------------------------------------------------------------
def _launches():
    from gss import _lib
    return _lib.stat("gemm_launches_128"), _lib.stat("gemm_launches_64")


def _assert_ran(tile, before, n=1):
    """The counter rule: since `before`, `n` products went to the `tile`-tile kernel and none to the other one."""
    after = _launches()
    got = (after[0] - before[0], after[1] - before[1])
    assert got == ((n, 0) if tile == 128 else (0, n)), "(128-tile, 64-tile) launches %r, meant %d on %d" % (got, n, tile)


def _draw(kind, rng, *shape):
    """"int": integers in -8 .. 8 (every partial sum is an integer far below 2^53: exact in any order);
    "normal": standard normals (the rounded comparison)."""
    if kind == "int":
        return rng.integers(-8, 9, size=shape).astype(np.float64)
    return rng.normal(size=shape)


def _place(X, cm, ld=None, off=0, pad=np.nan):
    """X on the device, column-major when `cm`, with leading dimension `ld` and `off` elements in front of it; what lies
    between the lines is `pad` (NaN for operands: a load that strays into it shows in the result).
    Returns (whole buffer, view that starts at X(0, 0), (row stride, column stride))."""
    import torch
    r, c = X.shape
    lead, nline = (r, c) if cm else (c, r)
    ld = lead if ld is None else ld
    assert ld >= lead
    buf = np.full(off + nline * ld, pad)
    buf[off:].reshape(nline, ld)[:, :lead] = X.T if cm else X
    t = torch.as_tensor(buf, device="cuda")
    return t, t[off:], ((1, ld) if cm else (ld, 1))


def _fetch(t, shape, cm, ld=None, off=0, pad=None):
    """The matrix back from a buffer laid out by `_place`; with `pad`, whatever lies between the lines still holds it."""
    r, c = shape
    lead, nline = (r, c) if cm else (c, r)
    ld = lead if ld is None else ld
    buf = t.cpu().numpy()
    v = buf[off:].reshape(nline, ld)
    if pad is not None:
        assert np.all(v[:, lead:] == pad) and np.all(buf[:off] == pad)
    return v[:, :lead].T if cm else v[:, :lead]


def _same(kind, got, ref, scale, K):
    if kind == "int":
        assert np.array_equal(got, ref)
    else:
        assert np.max(np.abs(got - ref) / scale) < 1e-14 * K


def _even(n):
    return n + (n & 1)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("K", [16, 48, 129, 1024])
@pytest.mark.parametrize("M,N", [(2048, 2048), (1990, 2041), (3703, 990)])
def test_gemm_128_tile_full_products(M, N, K, kind):
    """Column-major A, row-major B with even leading dimensions (the layout of the factorisations' products): with K a
    multiple of 16 the interior tiles stage with 16-byte loads and the ragged edge tiles with checked scalar loads in
    the same launch; K = 129 takes the scalar loads everywhere and ends on a partial k-step."""
    rng = np.random.default_rng(M + 3 * N + 7 * K)
    A, B = _draw(kind, rng, M, K), _draw(kind, rng, K, N)
    _, vA, sa = _place(A, True, _even(M))
    _, vB, sb = _place(B, False, _even(N))
    tD, vD, sd = _place(np.zeros((M, N)), True, M + 3, pad=7.0)
    before = _launches()
    _gemm(M, N, K, vA, sa, vB, sb, vD, sd)
    _assert_ran(128, before)
    _same(kind, _fetch(tD, (M, N), True, M + 3, pad=7.0), A @ B, np.abs(A) @ np.abs(B), K)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("K", [48, 129])
def test_gemm_128_tile_all_layouts(K, kind):
    """The eight storage layouts of A, B and D (the four <A_ICONTIG, B_JCONTIG> instantiations of the 128-tile kernel) on
    a product that is ragged in both directions."""
    M, N = 1990, 2041
    rng = np.random.default_rng(K)
    A, B = _draw(kind, rng, M, K), _draw(kind, rng, K, N)
    ref, scale = A @ B, np.abs(A) @ np.abs(B)
    for a_cm in (False, True):
        for b_cm in (False, True):
            for d_cm in (False, True):
                _, vA, sa = _place(A, a_cm)
                _, vB, sb = _place(B, b_cm)
                tD, vD, sd = _place(np.zeros((M, N)), d_cm)
                before = _launches()
                _gemm(M, N, K, vA, sa, vB, sb, vD, sd)
                _assert_ran(128, before)
                _same(kind, _fetch(tD, (M, N), d_cm), ref, scale, K)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("what", ["odd_lda", "odd_ldb", "offset_a", "offset_b"])
def test_gemm_128_tile_operands_that_forbid_16_byte_loads(what, kind):
    """(2048, 2048, 48) in the layout that stages with 16-byte loads, except for one thing: an odd leading dimension,
    or an operand that starts 8 bytes off a 16-byte boundary."""
    M = N = 2048
    K = 48
    rng = np.random.default_rng(len(what))
    A, B = _draw(kind, rng, M, K), _draw(kind, rng, K, N)
    _, vA, sa = _place(A, True, M + 1 if what == "odd_lda" else M + 2, off=1 if what == "offset_a" else 0)
    _, vB, sb = _place(B, False, N + 1 if what == "odd_ldb" else N + 2, off=1 if what == "offset_b" else 0)
    assert (vA.data_ptr() % 16 == 8) == (what == "offset_a") and (vB.data_ptr() % 16 == 8) == (what == "offset_b")
    tD, vD, sd = _place(np.zeros((M, N)), True)
    before = _launches()
    _gemm(M, N, K, vA, sa, vB, sb, vD, sd)
    _assert_ran(128, before)
    _same(kind, _fetch(tD, (M, N), True), A @ B, np.abs(A) @ np.abs(B), K)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("M,N,K", [(2816, 2816, 1024), (2816, 2816, 129), (3250, 1500, 1024), (3250, 1500, 129)])
def test_gemm_128_tile_lower_only_with_alpha_beta(M, N, K, kind):
    """D <- D - A B on the tiles on and below the block diagonal (the trailing updates; 3 250 x 1 500 has more row
    tiles than column tiles, the full rows below the block triangle): the lower triangle equals the reference, and
    the 128 x 128 tiles strictly above the block diagonal keep D's old bits."""
    rng = np.random.default_rng(M + N + K)
    A, B, D0 = _draw(kind, rng, M, K), _draw(kind, rng, K, N), _draw(kind, rng, M, N)
    _, vA, sa = _place(A, True)
    _, vB, sb = _place(B, False)
    tD, vD, sd = _place(D0, True, M + 2, pad=7.0)
    before = _launches()
    _gemm(M, N, K, vA, sa, vB, sb, vD, sd, alpha=-1.0, beta=1.0, lower=1)
    _assert_ran(128, before)
    got = _fetch(tD, (M, N), True, M + 2, pad=7.0)
    i, j = np.arange(M)[:, None], np.arange(N)[None, :]
    low = np.broadcast_to(i >= j, (M, N))
    above = np.broadcast_to(j // 128 > i // 128, (M, N))
    assert np.array_equal(got[above], D0[above])
    _same(kind, got[low], (D0 - A @ B)[low], (np.abs(A) @ np.abs(B))[low], K)


# operand shapes of the callers: the panel solve P = A21 Wk' (Wk' upper triangular, M >> N = K), the recursion's
# L21 W (W lower triangular) and W22 T with M = K (W22 lower triangular on the left)
@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("mode,M,N,K,tile", [
    (1, 4096, 1024, 1024, 128), (1, 3990, 1000, 1000, 128), (1, 300, 260, 260, 64),
    (2, 4096, 1024, 1024, 128), (2, 3990, 1000, 1000, 128), (2, 300, 260, 260, 64),
    (4, 4096, 1024, 4096, 128), (4, 3990, 1024, 3990, 128), (4, 300, 260, 300, 64)])
def test_gemm_zero_structure_modes(mode, M, N, K, tile, kind):
    """`lower_only` bits 1..3 tell the kernel where an operand is zero, so that it skips those k-tiles (and walks the
    grid by columns for the two B modes).  The operand carries exact zeros there and the reference is the plain full
    product: a k-tile skipped that should not be, or a tile computed for the wrong place, shows.  Sizes that are
    multiples of 16 stage with 16-byte loads, the others end on a partial k-step.  No caller combines a mode with the
    lower-tiles-only bit, so neither does this test."""
    rng = np.random.default_rng(mode * 1000 + M + K)
    A, B = _draw(kind, rng, M, K), _draw(kind, rng, K, N)
    if mode == 1:
        B = np.triu(B)                        # B(k, j) = 0 for k > j, stored as the lower-triangular Wk (B = Wk')
        b_cm = False
    elif mode == 2:
        B = np.tril(B)                        # B(k, j) = 0 for k < j: a column-major lower-triangular factor
        b_cm = True
    else:
        A = np.tril(A)                        # A(i, k) = 0 for k > i
        b_cm = True
    _, vA, sa = _place(A, True)
    _, vB, sb = _place(B, b_cm)
    tD, vD, sd = _place(np.zeros((M, N)), True)
    before = _launches()
    _gemm(M, N, K, vA, sa, vB, sb, vD, sd, lower=mode << 1)
    _assert_ran(tile, before)
    _same(kind, _fetch(tD, (M, N), True), A @ B, np.maximum(np.abs(A) @ np.abs(B), 1e-300), K)


@pytest.mark.parametrize("kind", ["int", "normal"])
@pytest.mark.parametrize("n,c0,k,R,tile", [(4374, 384, 896, 1024, 128), (4374, 384, 820, 1024, 128),
                                           (5300, 896, 896, 100, 64), (5300, 4480, 820, 100, 64)])
def test_gemm_column_block_of_a_triangular_factor(n, c0, k, R, tile, kind):
    """One column block of the split product Y = L W (gss_lugs_realize): the operands are views into larger arrays,
    A = L + c0 + c0 * n (rows c0 .. n - 1, columns c0 .. c0 + k - 1, lower triangular on the left), B = W + c0,
    D = Y + c0, all with the leading dimension n of the whole.  Rows above c0 of Y are not touched."""
    rng = np.random.default_rng(n + c0 + k)
    L, W = np.tril(_draw(kind, rng, n, n)), _draw(kind, rng, n, R)
    _, vL, sl = _place(L, True)
    _, vW, sw = _place(W, True)
    tY, vY, sy = _place(np.full((n, R), 7.0), True)
    before = _launches()
    _gemm(n - c0, R, k, vL[c0 + c0 * n:], sl, vW[c0:], sw, vY[c0:], sy, lower=4 << 1)
    _assert_ran(tile, before)
    Y = _fetch(tY, (n, R), True)
    assert np.all(Y[:c0] == 7.0)
    Ab, Bb = L[c0:, c0:c0 + k], W[c0:c0 + k]
    _same(kind, Y[c0:], Ab @ Bb, np.maximum(np.abs(Ab) @ np.abs(Bb), 1e-300), k)


@pytest.mark.parametrize("n", [1, 7, 64, 65, 200, 1000, 1537])
def test_potrf_and_trtri(n):
    import torch
    from gss import _lib
    l = _lib.lib()
    rng = np.random.default_rng(n)
    G = rng.normal(size=(n, n + 8))
    A = G @ G.T / n + np.eye(n)
    lda = n + 3
    buf = np.zeros((n, lda))
    buf[:, :n] = A                                            # row r of buf = column r (A symmetric)
    dA = _t(buf)
    _lib.check(l.gss_dev_potrf(_lib.ptr(dA), n, lda, _lib.current_stream()))
    L = np.tril(dA.cpu().numpy()[:, :n].T)
    Lref = np.linalg.cholesky(A)
    assert np.max(np.abs(L - Lref)) < 1e-10 * np.max(np.abs(Lref))
    dW = torch.full((n, lda), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(l.gss_dev_trtri(_lib.ptr(dA), n, lda, _lib.ptr(dW), lda, _lib.current_stream()))
    W = dW.cpu().numpy()[:, :n].T
    assert np.array_equal(np.triu(W, 1), np.zeros((n, n)))
    assert np.max(np.abs(W @ Lref - np.eye(n))) < 1e-9


@pytest.mark.parametrize("n", [5, 128, 129, 256, 257, 300, 384, 385, 1000, 1024, 1025, 1600, 2048])
def test_potrf_inverse_single_launch_panel(n):
    """Factor and inverse together (the kriging fit, the LUGS blocks): blocks of 257 ... 1 024 rows run as one
    cooperative launch (potrf_inv_panel_kernel, grid barriers between its phases), larger ones split down to it,
    smaller ones are the 64 / 128 leaves.  Partial last blocks, leading dimensions that are not multiples of
    anything, and what lies outside the n x n blocks is left alone."""
    import torch
    from gss import _lib
    l = _lib.lib()
    rng = np.random.default_rng(n)
    G = rng.normal(size=(n, n + 8))
    A = G @ G.T / n + np.eye(n)
    lda, ldw = n + 3, n + 5
    buf = np.full((n + 2, lda), 9.0)
    buf[:n, :n] = A
    dA = _t(buf)
    dW = torch.full((n + 2, ldw), 7.0, dtype=torch.float64, device="cuda")
    _lib.check(l.gss_dev_potrf_inverse(_lib.ptr(dA), n, lda, _lib.ptr(dW), ldw, _lib.current_stream()))
    gotA, gotW = dA.cpu().numpy(), dW.cpu().numpy()
    L = np.tril(gotA[:n, :n].T)
    Lref = np.linalg.cholesky(A)
    assert np.max(np.abs(L - Lref)) < 1e-10 * np.max(np.abs(Lref))
    W = gotW[:n, :n].T
    assert np.array_equal(np.triu(W, 1), np.zeros((n, n)))
    assert np.max(np.abs(W @ Lref - np.eye(n))) < 1e-9
    assert np.all(gotA[n:, :] == 9.0) and np.all(gotA[:, n:] == 9.0)
    assert np.all(gotW[n:, :] == 7.0) and np.all(gotW[:, n:] == 7.0)


def test_potrf_inverse_launch_per_block_path_stays_alive():
    """GSS_PANEL_MAX=0 switches the single-launch kernel off (the path a process falls back to when a launch reports
    that its workgroups did not all arrive): same answers from the launch-per-block recursion.  The switch is read once
    per process, hence the subprocess."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "from gss import _lib\n"
        "l = _lib.lib()\n"
        "for n in (700, 1000, 1537):\n"
        "    rng = np.random.default_rng(n)\n"
        "    G = rng.normal(size=(n, n + 8)); A = G @ G.T / n + np.eye(n)\n"
        "    dA = torch.from_numpy(A.copy()).cuda(); dW = torch.zeros((n, n), dtype=torch.float64, device='cuda')\n"
        "    _lib.check(l.gss_dev_potrf_inverse(_lib.ptr(dA), n, n, _lib.ptr(dW), n, _lib.current_stream()))\n"
        "    L = np.linalg.cholesky(A); W = dW.cpu().numpy().T\n"
        "    assert np.max(np.abs(np.tril(dA.cpu().numpy().T) - L)) < 1e-10 * np.max(np.abs(L))\n"
        "    assert np.max(np.abs(W @ L - np.eye(n))) < 1e-9\n"
        "print('RECURSION OK')\n"
    ) % (root, os.path.join(root, "geostatssolvers.jl_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSS_PANEL_MAX="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "RECURSION OK" in r.stdout, r.stderr[-2000:]


def test_recovery_when_the_single_launch_kernel_gives_up():
    """A launch whose workgroups do not all arrive within the bounded spin reports -1 (GSS_PANEL_FAIL=1 fakes exactly
    that for the first launch of the process): the kriging fit retries on the launch-per-block path by itself and the
    results are the usual ones; gss_lugs_create runs its preprocess a second time by itself."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, gss\n"
        "from gss import _lib\n"
        "from gss.engine import KrigHandle, LUGSHandle, OK\n"
        "from oracle import kriging as K\n"
        "from oracle.variogram import Variogram\n"
        "rng = np.random.default_rng(0)\n"
        "x = rng.uniform(0, 100, (600, 3)); z = rng.normal(size=600); x0 = rng.uniform(0, 100, (50, 3))\n"
        "h = KrigHandle(gss.MaternVariogram(range=30.0, order=1.5), OK, x, z)\n"
        "mu, var, st = h.predict_global(x0)\n"
        "ref = K.predict(K.fit(K.OK, Variogram('matern', range=30.0, nu=1.5), x, z), x0)\n"
        "assert np.max(np.abs(mu - ref[0])) < 1e-9 and np.max(np.abs(var - ref[1])) < 1e-9\n"
        "print('KRIG RECOVERED')\n"
    ) % (root, os.path.join(root, "geostatssolvers.jl_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSS_PANEL_FAIL="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "KRIG RECOVERED" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    code2 = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, gss\n"
        "from gss import _lib\n"
        "from gss.engine import LUGSHandle\n"
        "cent = gss.CartesianGrid(40, 30).centroids()\n"
        "dl = np.arange(0, 1200, 3)[:300]; z1 = np.random.default_rng(1).normal(size=300)\n"
        "h = LUGSHandle(gss.SphericalVariogram(range=8.0, nugget=0.05), cent, dl, z1)\n"
        "r = h.realize(1, 0, 2)\n"
        "assert np.array_equal(r[0][:, dl] if isinstance(r, tuple) else r[:, dl], np.tile(z1, (2, 1)))\n"
        "print('LUGS RECOVERED')\n"
    ) % (root, os.path.join(root, "geostatssolvers.jl_amd"))
    r = subprocess.run([sys.executable, "-c", code2], env=dict(os.environ, GSS_PANEL_FAIL="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "LUGS RECOVERED" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_potrf_inverse_panel_reports_the_pivot():
    from gss import _lib
    l = _lib.lib()
    n = 700
    A = np.eye(n)
    A[533, 533] = -2.0
    dA, dW = _t(A), _t(np.zeros((n, n)))
    code = l.gss_dev_potrf_inverse(_lib.ptr(dA), n, n, _lib.ptr(dW), n, _lib.current_stream())
    assert code == _lib.ERR_NOT_POSDEF and "pivot at row 533" in _lib.last_error()


def test_potrf_reports_indefinite():
    from gss import _lib
    l = _lib.lib()
    A = np.eye(100)
    A[70, 70] = -1.0
    dA = _t(A)
    code = l.gss_dev_potrf(_lib.ptr(dA), 100, 100, _lib.current_stream())
    assert code == _lib.ERR_NOT_POSDEF and "pivot at row 70" in _lib.last_error()


@pytest.mark.parametrize("n", [1, 7, 32, 33, 100, 257, 1500, 2500, 4133])
def test_getrf_unit_lower_matches_lapack(n):
    """gss_dev_getrf_l: `lu(A).L` with LAPACK's pivoting rule (first row of maximal |a|), on matrices that do pivot.
    Beyond 2 048 rows the 32-column panels run on a grid of workgroups with one barrier per column (lu.hip); 4 133 is
    ragged against the 128-column outer panels, the 32-column panels and the 1 024-row workgroups."""
    import scipy.linalg as sla
    import torch
    from gss import _lib
    rng = np.random.default_rng(n)
    A = rng.normal(size=(n, n)) + 0.5 * np.eye(n)
    dA = _t(A.T)                                     # column-major image
    _lib.check(_lib.lib().gss_dev_getrf_l(_lib.ptr(dA), n, n, _lib.current_stream()))
    torch.cuda.synchronize()
    L = dA.cpu().numpy().T
    P, Lref, U = sla.lu(A)
    assert not np.array_equal(P, np.eye(n)) or n < 3
    assert np.max(np.abs(L - Lref)) < 1e-10 * max(1.0, np.max(np.abs(np.linalg.inv(U))) * 1e-3)


def test_lu_grid_panel_gives_up_cleanly():
    """GSS_LU_PANEL_FAIL=1 gives the first grid panel of the process no patience at its barriers, so its workgroups
    really leave through the give-up path of `getrf_panel_grid_kernel` (lu.hip): the verdict must be "gave up" (-1), never
    a spurious "exactly singular matrix" from candidate records that nobody wrote, the later panels of the call must not
    wait again, and the message must say that the matrix was overwritten.  The second call of the process runs on the
    single-workgroup panels and matches LAPACK; `gss_lugs_create(factorization = lu)` retries by itself."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, time\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, scipy.linalg as sla, gss\n"
        "from gss import _lib\n"
        "n = 2500\n"
        "A = np.random.default_rng(3).normal(size=(n, n)) + 0.5 * np.eye(n)\n"
        "dA = torch.as_tensor(np.ascontiguousarray(A.T), device='cuda')\n"
        "t = time.time()\n"
        "rc = _lib.lib().gss_dev_getrf_l(_lib.ptr(dA), n, n, _lib.current_stream())\n"
        "assert rc == _lib.ERR_HIP, rc\n"
        "msg = _lib.last_error()\n"
        "assert 'gave up' in msg and 'restore the input' in msg and 'singular' not in msg, msg\n"
        "assert time.time() - t < 20.0\n"
        "dA = torch.as_tensor(np.ascontiguousarray(A.T), device='cuda')\n"
        "_lib.check(_lib.lib().gss_dev_getrf_l(_lib.ptr(dA), n, n, _lib.current_stream()))\n"
        "torch.cuda.synchronize()\n"
        "P, Lref, U = sla.lu(A)\n"
        "assert np.max(np.abs(dA.cpu().numpy().T - Lref)) < 1e-10\n"
        "print('GETRF RECOVERED')\n"
    ) % (root, os.path.join(root, "geostatssolvers.jl_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GSS_LU_PANEL_FAIL="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "GETRF RECOVERED" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    code2 = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, gss\n"
        "from gss.engine import LUGSHandle\n"
        "from oracle import lugs as OL\n"
        "from oracle.variogram import Variogram\n"
        "cent = gss.CartesianGrid(60, 50).centroids()\n"
        "h = LUGSHandle(gss.SphericalVariogram(range=8.0, nugget=0.05), cent, np.zeros(0, np.int64), np.zeros(0),\n"
        "               factorization='lu')\n"
        "L22, d2 = h.factor()\n"
        "pre = OL.preprocess(Variogram('spherical', range=8.0, nugget=0.05), cent, factorization='lu')\n"
        "assert np.max(np.abs(L22 - pre.L22)) < 1e-9\n"
        "print('LUGS LU RECOVERED')\n"
    ) % (root, os.path.join(root, "geostatssolvers.jl_amd"))
    r = subprocess.run([sys.executable, "-c", code2], env=dict(os.environ, GSS_LU_PANEL_FAIL="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "LUGS LU RECOVERED" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_single_launch_panel_beside_a_callers_own_kernels():
    """The single-launch factor-and-inverse kernel needs its 64 workgroups resident together, a whole CU each.  The
    library's own launch order guarantees that; a CALLER's kernels on another stream (here: a chain of large FP64
    matrix products from torch, LDS-heavy workgroups that keep every CU busy) can delay their arrival.  Whatever happens
    -- the panel squeezes in, or its bounded wait ends and the fit repeats on the launch-per-block path -- the
    estimates must be the usual ones and the call must return; the child prints what happened and what it cost
    (recorded in profiles/)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, time\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, gss\n"
        "from gss import _lib\n"
        "from gss.engine import KrigHandle, OK\n"
        "from oracle import kriging as K\n"
        "from oracle.variogram import Variogram\n"
        "rng = np.random.default_rng(0)\n"
        "x = rng.uniform(0, 100, (1000, 3)); z = rng.normal(size=1000); x0 = rng.uniform(0, 100, (400, 3))\n"
        "ref = K.predict(K.fit(K.OK, Variogram('matern', range=30.0, nu=1.5), x, z), x0)\n"
        "vg = gss.MaternVariogram(range=30.0, order=1.5)\n"
        "def fit_predict():\n"
        "    t0 = time.perf_counter()\n"
        "    h = KrigHandle(vg, OK, x, z)\n"
        "    mu, var, st = h.predict_global(x0)\n"
        "    torch.cuda.synchronize()\n"
        "    dt = time.perf_counter() - t0\n"
        "    h.close()\n"
        "    assert np.max(np.abs(mu - ref[0])) < 1e-9 and np.max(np.abs(var - ref[1])) < 1e-9\n"
        "    return dt\n"
        "fit_predict()\n"
        "alone = min(fit_predict() for _ in range(3))\n"
        "a = torch.randn(6144, 6144, dtype=torch.float64, device='cuda')\n"
        "side = torch.cuda.Stream()\n"
        "beside = []\n"
        "for trial in range(6):\n"
        "    with torch.cuda.stream(side):\n"
        "        for _ in range(8):\n"
        "            b = a @ a\n"
        "    beside.append(fit_predict())\n"
        "    torch.cuda.synchronize()\n"
        "print('FOREIGN alone %%.2f ms, beside the products %%s ms, give-ups %%d' %% (alone * 1e3, ' '.join('%%.2f' %% (t * 1e3) for t in beside), _lib.stat('panel_giveups')))\n"
    ) % (root, os.path.join(root, "geostatssolvers.jl_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FOREIGN alone" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    print([l for l in r.stdout.splitlines() if l.startswith("FOREIGN")][0])
