"""numpy restatement of the SPDE operators, the reference's dense method and the Jacobi-CG the device runs (gss.h,
"SPDEGS"; src/simulation/spde.jl of the reference), and the four small meshes the SPDE tests share."""
import functools
import math

import numpy as np

EPS = np.finfo(np.float64).eps


# ---- operators -----------------------------------------------------------------------------------------------------
def tau2_of(sill, range):
    """spde.jl:57-63 with d = 2, alpha = 2, nu = 1: sill^2 kappa^(2 nu) (4 pi)^(d/2) Gamma(alpha) / Gamma(nu)."""
    kappa = 1.0 / range
    return sill ** 2 * kappa ** 2 * (4.0 * math.pi) * math.gamma(2.0) / math.gamma(1.0)


def operators(V, T, sill=1.0, range=1.0):
    """Dense cotangent Laplace matrix B, lumped masses m, S = kappa^2 diag(m) - B and tau^2.  Triangle (a, b, c) with
    area A: cot_c = ((a - c) . (b - c)) / (2 A) adds +cot_c / 2 to B[a][b], B[b][a] and -cot_c / 2 to B[a][a], B[b][b];
    A / 3 goes to m[a]; cyclically.  Contributions are added in triangle order."""
    V = np.asarray(V, dtype=np.float64)
    P = np.zeros((V.shape[0], 3))
    P[:, :V.shape[1]] = V
    nv = V.shape[0]
    B, m = np.zeros((nv, nv)), np.zeros(nv)
    for tri in np.asarray(T):
        p = P[tri]
        u, v = p[1] - p[0], p[2] - p[0]
        cx, cy, cz = u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]
        area = 0.5 * math.sqrt((cx * cx + cy * cy) + cz * cz)
        for k in (0, 1, 2):
            c, a, b = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
            da, db = P[a] - P[c], P[b] - P[c]
            w = 0.5 * (((da[0] * db[0] + da[1] * db[1]) + da[2] * db[2]) / (2.0 * area))
            B[a, b] += w
            B[b, a] += w
            B[a, a] += -w
            B[b, b] += -w
            m[a] += area / 3.0
    kappa2 = (1.0 / range) * (1.0 / range)
    S = -B
    S[np.diag_indices(nv)] = kappa2 * m - np.diag(B)
    return B, m, S, tau2_of(sill, range)


def reference_cov(V, T, sill, range):
    """inv(Q) with Q = A'A / tau^2, A = kappa^2 I - inv(M) B: exactly what spde.jl:37-39, 56-64 forms."""
    B, m, _, tau2 = operators(V, T, sill, range)
    A = (1.0 / range) ** 2 * np.eye(len(m)) - np.diag(1.0 / m) @ B
    return np.linalg.inv(A.T @ A / tau2)


def rhs_scale(m, tau2, lumped):
    """b = scale * w: tau m for the reference's w ~ N(0, I), tau sqrt(m) for the lumped form."""
    return math.sqrt(tau2) * (np.sqrt(m) if lumped else m)


def cg(S, b, rtol=1e-10, maxiter=20000):
    """Jacobi-preconditioned CG on the columns of b (nv,) or (nv, ncols), every column with its own scalars; a column
    whose recursive residual satisfies ||r|| <= rtol ||b|| is frozen.  Returns (x, iterations per column)."""
    one = b.ndim == 1
    b = b.reshape(len(b), -1)
    dinv = 1.0 / np.diag(S)
    x, r = np.zeros_like(b), b.copy()
    p = np.zeros_like(b)
    bn2 = (b * b).sum(axis=0)
    rho = np.ones(b.shape[1])
    iters = np.zeros(b.shape[1], dtype=np.int64)
    done = np.zeros(b.shape[1], dtype=bool)
    for k in range(maxiter + 1):
        z = dinv[:, None] * r
        rz, rr = (r * z).sum(axis=0), (r * r).sum(axis=0)
        live = ~done
        iters[live] = k
        done |= live & (rr <= rtol * rtol * bn2)
        live = ~done
        if not live.any() or k == maxiter:
            break
        beta = np.where(k == 0, 0.0, rz[live] / rho[live])
        rho[live] = rz[live]
        p[:, live] = z[:, live] + beta * p[:, live]
        Ap = S @ p[:, live]
        alpha = rho[live] / (p[:, live] * Ap).sum(axis=0)
        x[:, live] += alpha * p[:, live]
        r[:, live] -= alpha * Ap
    return (x[:, 0], int(iters[0])) if one else (x, iters)


# ---- meshes --------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny, spacing=1.0):
    """nx x ny nodes, x fastest; every cell split along the diagonal from its lower left node."""
    X, Y = np.meshgrid(np.arange(nx) * spacing, np.arange(ny) * spacing, indexing="xy")
    V = np.stack([X.ravel(), Y.ravel()], axis=1)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="xy")
    n00 = (j * nx + i).ravel()
    n10, n01, n11 = n00 + 1, n00 + nx, n00 + nx + 1
    T = np.stack([np.stack([n00, n10, n11], axis=1), np.stack([n00, n11, n01], axis=1)], axis=1).reshape(-1, 3)
    return V, T.astype(np.int64)


def icosphere(subdivisions):
    """Unit icosphere: 10 * 4^s + 2 vertices, 20 * 4^s triangles."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    V = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    V = [np.array(v, dtype=np.float64) / math.sqrt(1.0 + g * g) for v in V]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdivisions):
        mid, T2 = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in T:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    return np.array(V), np.array(T, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices, triangles, sill, range) of the shared cases; none has a vertex count that is a multiple of 64.
    "jitter": 13 x 11 nodes moved by up to 0.3 spacings (obtuse triangles, negative cotangents), 143 vertices;
    "sphere": icosphere of two subdivisions in 3-D, 162 vertices; "fan": a hub shared by 40 triangles and its ring of
    40, 41 vertices; "strip": two triangles on four vertices."""
    if name == "jitter":
        V, T = grid_mesh(13, 11)
        V = V + np.random.default_rng(11).uniform(-0.3, 0.3, V.shape)
        out = V, T, 1.5, 4.0
    elif name == "sphere":
        out = icosphere(2) + (1.2, 0.5)
    elif name == "fan":
        ang = 2.0 * math.pi * np.arange(40) / 40
        V = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang)], axis=1)])
        T = np.array([(0, 1 + k, 1 + (k + 1) % 40) for k in range(40)], dtype=np.int64)
        out = V, T, 1.0, 0.5
    elif name == "strip":
        out = (np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.2]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64),
               2.0, 1.5)
    else:
        raise KeyError(name)
    for a in out[:2]:
        a.setflags(write=False)
    return out


MESHES = ("jitter", "sphere", "fan", "strip")


@functools.lru_cache(maxsize=None)
def dense(name):
    """operators() of a shared mesh, computed once."""
    V, T, sill, rng = mesh(name)
    out = operators(V, T, sill, rng)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def mixed_columns(name, lumped=False):
    """(5, nv) normals whose columns converge after different numbers of iterations: white noise, a zero column (done
    from the start), white noise, the constant that makes b = kappa^2 m (solution: the constant field), a spike."""
    V, _, _, rng = mesh(name)
    _, m, _, tau2 = dense(name)
    nv = V.shape[0]
    w = np.random.default_rng(5).normal(size=(5, nv))
    w[1] = 0.0
    w[3] = (1.0 / rng) ** 2 * m / rhs_scale(m, tau2, lumped)
    w[4] = 0.0
    w[4, nv // 2] = 1.0
    return w
