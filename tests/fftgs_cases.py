"""One run per compiled instantiation of the FFTGS kernels.

tests/test_fftgs_census.py holds this table against the kernels the compiler emitted into libgss_hip.so
(tools/kernel_census.py): every compiled kernel of FAMILIES has exactly one entry in CASES and every entry names a compiled
kernel, so an instantiation added to a `with_x_variant` / `with_axis_variant` switch (csrc/fftgs_fused.hip,
csrc/fftgs_generic.hip) or to `lmc_mix_launch` (csrc/fftgs_lmc.h) without a run fails on the CPU.  One pipeline run
launches several kernels, so the table has two parts: RUNS, the named runs, and CASES, which maps every key to the name
of a run that launches it or to UNREACHABLE("reason citing the dispatch line that rules the instantiation out").
tests/test_gpu_fftgs_matrix.py does every run on the device against the 80-bit restatement of tests/fftgs_matrix.py;
profiles/kernel_census_fftgs.txt is the kernel trace of that file alone.

Keys are (kernel family, template arguments as the demangler prints them).  The arguments:
 * ff_x_fwd2_kernel<SRC, ROWS, 256, LOGM>, gen_x_fwd_kernel<SRC, TG>: SRC 0 Philox uniforms, 1 the caller's uniforms
   (a realisation, seeded or from supplied noise), 2 the covariance, 3 the covariance at rotated lags (the spectrum of
   gss_fftgs_create; `h->rotated` in fftgs_spectrum_fused / fftgs_spectrum_generic);
 * <ROWS, 256, LOGM> of ff_x_fwd2_kernel / ff_x_inv2_kernel (with_x_variant, csrc/fftgs_fused.hip): <8, 256, 8> when
   `h->fg.l1 == 9` (n1 = 512), <8, 256, -1> when `h->x_rows == 8` (n1 <= 512 otherwise), <4, 256, -1> for n1 = 1024;
 * ff_axis2_kernel<MODE, TXLOG, NT, -1> / ff_axis2_fast_kernel<MODE, 3, 512, 9> (with_axis_variant): MODE 0 forward
   (spectrum, and P2 along y), 2 forward-phase-inverse (P3 along z), 1 inverse (P4 along y); 512-point lines take the
   fast kernel, lines of 1024 points tiles of four columns (`txy_log` / `txz_log` = 2), everything else <., 3, 512, -1>;
   ff_tile_fh2_kernel<TXLOG> follows `txz_log` (fftgs_tile_fused);
 * gen_x_*<TG>: `g_tg` of fftgs_setup_generic, true when the twiddle tables in LDS would leave at most two workgroups
   per CU (n1 / 2 = 2048: 96 KB with them, 32 KB without); gen_axis_kernel<MODE, TXLOG>: `g_txlog[axis]` = 2 for lines
   longer than 512 points (448 with a factor 7); gen_tile_fh_kernel<TXLOG> follows the last strided axis; `g_long`
   (a 2-D grid with n2 > 1024) takes the gen_long_* kernels and gen_tile_fh_long_kernel; a 1-D grid gen_phase1d_kernel;
 * fftgs_lmc_mix_kernel<NZ, VEC>: NZ by `lmc_mix_launch`, VEC = 2 when `vec` of lmc_mix_launch_nz holds (N even, 16-byte
   aligned slots), else 1.

Every run is small (at most 0.53 M cells) and is routed by its sizes and by GSS_FFTGS_PATH, which is read per
gss_fftgs_create; nothing depends on a switch that is read once per process.

The model.  The FP64 oracle (oracle/fftgs.py) must be quiet where the device is held to it: with the suite's usual
range = 0.2 n1, nugget = 0.05 its spectrum at 1024 x 16 x 16 is 6.8e-13 of max F off the 80-bit restatement, most of the
1e-12 the suite allows.  Every run here has a practical range of 8 cells, sill 1.4 and nugget 0.28 (a fifth of the sill:
the white floor keeps the smallest |FFT C| some 1e-2 of the largest, so sqrt|.| does not magnify the transform's rounding);
rotated runs have the ball RADII[d] on the frame ROT[d].  Gaussian models stay out (their 1e-6 rule has its own tests).
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

FAMILIES = (
    # fused pipeline (csrc/fftgs_fused.hip)
    "ff_x_fwd2_kernel", "ff_x_inv2_kernel", "ff_axis2_kernel", "ff_axis2_fast_kernel", "ff_tile_fh2_kernel", "ff_amp_kernel",
    # generic pipeline (csrc/fftgs_generic.hip)
    "gen_x_fwd_kernel", "gen_x_inv_kernel", "gen_axis_kernel", "gen_long_outer_kernel", "gen_long_inner_kernel",
    "gen_tile_fh_kernel", "gen_tile_fh_long_kernel", "gen_amp_kernel", "gen_phase1d_kernel",
    # the rocFFT pipeline's own kernels (csrc/fftgs_rocfft.hip) and what every pipeline shares (csrc/fftgs.hip)
    "fftgs_cov_kernel", "fftgs_cov_rot_kernel", "fftgs_amp_kernel", "fftgs_phase_kernel", "fftgs_scale_kernel",
    "fftgs_expand_kernel", "fftgs_apply_scale_kernel",
    # co-simulation (csrc/fftgs_lmc.h)
    "fftgs_lmc_mix_kernel",
)

SILL, NUGGET, RANGE, MEAN = 1.4, 0.28, 8.0, 0.3
RADII = {2: (8.0, 4.0), 3: (8.0, 5.0, 3.0)}


def _rot2(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s], [s, c]])


def _rot3(a, b, g):
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    Z = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]])
    Y = np.array([[cb, 0, sb], [0, 1.0, 0], [-sb, 0, cb]])
    X = np.array([[1.0, 0, 0], [0, cg, -sg], [0, sg, cg]])
    return Z @ Y @ X


ROT = {2: _rot2(0.5235987755982988), 3: _rot3(0.4, -0.7, 1.2)}


@dataclass(frozen=True)
class Run:
    dims: Tuple[int, ...]
    pipeline: str                                  # "fused" | "generic" | "rocfft": where the dispatch sends the grid
    path: Optional[str] = None                     # GSS_FFTGS_PATH, set before the handle is created
    spacing: Optional[Tuple[float, ...]] = None
    kind: str = "exponential"
    rotated: bool = False                          # the ball RADII[d] on the frame ROT[d] instead of the range RANGE
    nz: int = 0                                    # > 0: a co-simulation of nz variables (lmc_b0, lmc_b1, lmc_means)

    @property
    def model(self):
        """Keyword arguments of the model: sill and nugget, and the range or the radii of the ball."""
        kw = dict(sill=SILL, nugget=NUGGET)
        if self.rotated:
            kw["radii"] = RADII[len(self.dims)]
        else:
            kw["range"] = RANGE
        return kw

    @property
    def rotation(self):
        return ROT[len(self.dims)] if self.rotated else None


@dataclass(frozen=True)
class UNREACHABLE:
    reason: str


def _psd(n, seed, ridge):
    A = np.random.default_rng(seed).normal(size=(n, n))
    return A @ A.T / n + ridge * np.eye(n)


def lmc_b0(nz):
    """Nugget coefficients of the co-simulation runs: full rank, entries of order 0.1."""
    return 0.2 * _psd(nz, 100 + nz, 0.25)


def lmc_b1(nz):
    """Coefficients of the structure: full rank, entries of order 1."""
    return _psd(nz, 200 + nz, 0.1)


def lmc_means(nz):
    return np.arange(nz, dtype=np.float64) - 0.5 * nz + 0.25


# Error bars.  "oracle": the largest error of oracle.fftgs (FP64, complex pocketfft) against the 80-bit restatement of
# tests/fftgs_matrix.py over every run of RUNS, measured on the CPU with tools/fftgs_matrix_oracle.py -- the spectral
# amplitude F relative to max F, the realisations z (seeded and from supplied noise, co-simulated variables included)
# as an absolute error.  "bar" = 16 x that, the factor and the reasoning of kernel_cases.BARS: the device transforms
# real-to-complex, pass by pass in another order, and has its own exp, sqrt, rsqrt and sincos of 2.2e-16 relative
# error.  Every run's model keeps the oracle within 1/16 of the tolerances the suite already holds (1e-12 of max F and
# 1e-9 for z, tests/test_gpu_fftgs.py), so no bar is looser than those; tests/test_fftgs_census.py asserts both.
TOL = {"F": 1e-12, "z": 1e-9}
BARS = {
    "F": {"oracle": 3.692e-14, "bar": 5.908e-13},
    "z": {"oracle": 1.203e-13, "bar": 1.925e-12},
}

_FUSED = dict(pipeline="fused", path="fused")

RUNS = {
    # ---- fused pipeline.  GSS_FFTGS_PATH=fused: without it the 12 MiB rule of fftgs_setup_fused leaves every one of
    # these grids to the generic passes.  Each run launches, for its x variant V = <ROWS, 256, LOGM>,
    # ff_x_fwd2_kernel<2 or 3, V> (spectrum; 3 when `h->rotated`), <0, V> (seeded realisation, fftgs_fused_p1 without
    # noise), <1, V> (supplied noise) and ff_x_inv2_kernel<V>; for its y lines ff_axis2*<0, ..> (spectrum and P2) and
    # <1, ..> (P4); for its z lines <0, ..> (spectrum) and <2, ..> (P3); ff_amp_kernel; ff_tile_fh2_kernel<txz_log>.
    # V = <8, 256, -1>: x_rows == 8 (M = 16 <= 256) and l1 = 5; 16-point y and z lines: txy_log = txz_log = 3 and
    # logL = 4, so ff_axis2_kernel<0 | 1 | 2, 3, 512, -1> and ff_tile_fh2_kernel<3>
    "fused_32x16x16": Run((32, 16, 16), **_FUSED),
    "fused_32x16x16_rot": Run((32, 16, 16), rotated=True, **_FUSED),
    # V = <8, 256, 8>: `h->fg.l1 == 9`, the first line of with_x_variant
    "fused_512x16x16": Run((512, 16, 16), **_FUSED),
    "fused_512x16x16_rot": Run((512, 16, 16), rotated=True, **_FUSED),
    # V = <4, 256, -1>: M = 512 > 256 gives x_rows = 4, l1 = 10
    "fused_1024x16x16": Run((1024, 16, 16), **_FUSED),
    "fused_1024x16x16_rot": Run((1024, 16, 16), rotated=True, **_FUSED),
    # n2 = 1024 > 512: txy_log = 2, with_axis_variant's last line: ff_axis2_kernel<0, 2, 256, -1> (spectrum, P2) and
    # <1, 2, 256, -1> (P4) along y; txz_log = 3 along z (16 points), whose 8-column kernel has the LDS bound of the
    # 1024-point line (lmax in fftgs_setup_fused): the mixed case
    "fused_32x1024x16": Run((32, 1024, 16), **_FUSED),
    # n3 = 1024: txz_log = 2: ff_axis2_kernel<0, 2, 256, -1> (spectrum) and <2, 2, 256, -1> (P3) along z and
    # ff_tile_fh2_kernel<2> (`h->txz_log == 3` fails in fftgs_tile_fused); txy_log = 3
    "fused_32x16x1024": Run((32, 16, 1024), **_FUSED),
    # 512-point lines: `txlog == 3 && logL == 9`, the first line of with_axis_variant: ff_axis2_fast_kernel<0, 3, 512, 9>
    # and <1, 3, 512, 9> along y (no slab order: can_slab of fftgs_fused_rest needs l2 == 9 and l3 == 9)
    "fused_32x512x16": Run((32, 512, 16), **_FUSED),
    # ... and along z: ff_axis2_fast_kernel<0, 3, 512, 9> (spectrum) and <2, 3, 512, 9> (P3)
    "fused_32x16x512": Run((32, 16, 512), **_FUSED),

    # ---- generic pipeline (fftgs_setup_generic takes these by their sizes; n1 even, no power-of-two 3-D grid).  Each run
    # launches gen_x_fwd_kernel<2 or 3, TG> (spectrum), <0, TG> (seeded), <1, TG> (supplied noise), gen_x_inv_kernel<TG>
    # and gen_amp_kernel.
    # n3 = 600 > 512: g_txlog[2] = 2: gen_axis_kernel<0, 2> (spectrum) and <2, 2> (fftgs_fields_generic, ndim == 3)
    # along z and gen_tile_fh_kernel<2>; n2 = 18: g_txlog[1] = 3: gen_axis_kernel<0, 3> and <1, 3> along y; g_tg false
    # (n1 / 2 = 10)
    "gen_20x18x600": Run((20, 18, 600), "generic"),
    # n2 = 600: g_txlog[1] = 2: gen_axis_kernel<0, 2> and <1, 2> (the inverse y pass, 3-D grids only) along y;
    # gen_axis_kernel<0, 3> and <2, 3> along z and gen_tile_fh_kernel<3>
    "gen_20x600x18": Run((20, 600, 18), "generic"),
    # n1 / 2 = 2048: one line per workgroup, 96 KB of LDS with the tables against 32 KB without: g_tg true,
    # with_x_variant gives gen_x_fwd_kernel<0 | 1 | 2, true> and gen_x_inv_kernel<true>; a 2-D grid: gen_axis_kernel<0, 3>
    # (spectrum) and <2, 3> (the last branch of fftgs_fields_generic), gen_tile_fh_kernel<3> on axis 1
    "gen_4096x16": Run((4096, 16), "generic"),
    # ... `h->rotated`: gen_x_fwd_kernel<3, true>
    "gen_4096x16_rot": Run((4096, 16), "generic", rotated=True),
    # ndim == 1: gen_phase1d_kernel between the x passes (g_tg true as above), no strided pass, no tiled amplitudes
    "gen_4096": Run((4096,), "generic"),
    # n1 / 2 = 50: sixteen lines per workgroup, eleven workgroups per CU with the tables: g_tg false:
    # gen_x_fwd_kernel<0 | 1 | 2, false>, gen_x_inv_kernel<false>; unequal spacing
    "gen_100x100": Run((100, 100), "generic", spacing=(0.5, 1.0)),
    # ... `h->rotated`: gen_x_fwd_kernel<3, false>
    "gen_100x100_rot": Run((100, 100), "generic", rotated=True),
    # a 2-D grid with n2 = 2048 > 1024: `g_long`: gen_long_outer_kernel<false>, gen_long_inner_kernel<0> (spectrum,
    # gen_launch_long<0>), gen_long_inner_kernel<2> and gen_long_outer_kernel<true> (gen_launch_long<2>),
    # gen_tile_fh_long_kernel
    "gen_64x2048": Run((64, 2048), "generic"),

    # ---- rocFFT pipeline: n1 odd, which fftgs_setup_generic refuses (`g.n1 & 1`) and fftgs_setup_fused too (not a power
    # of two).  fftgs_cov_kernel or, with `h->rotated`, fftgs_cov_rot_kernel (fftgs_spectrum_rocfft), fftgs_amp_kernel,
    # fftgs_phase_kernel (fftgs_fields_rocfft).  Every run of every pipeline launches fftgs_scale_kernel and
    # fftgs_apply_scale_kernel (gss_fftgs_create) and fftgs_expand_kernel (gss_fftgs_spectrum).
    "rocfft_15x13x11": Run((15, 13, 11), "rocfft", spacing=(1.0, 2.0, 0.5)),
    "rocfft_15x13x11_rot": Run((15, 13, 11), "rocfft", rotated=True),
}

# ---- co-simulation: fftgs_lmc_mix_kernel<NZ, VEC>, NZ by the switch of lmc_mix_launch.  24 x 20 (generic passes): N = 480
# is even and the slots are 16-byte aligned (the ring's chunk, the staged normals), so `vec` of lmc_mix_launch_nz holds
# and VEC = 2; 15 x 13 and (101,) (rocFFT): N odd, VEC = 1.
for _nz in range(1, 9):
    RUNS["lmc%d_24x20" % _nz] = Run((24, 20), "generic", nz=_nz)
    RUNS["lmc%d_%s" % (_nz, "15x13" if _nz % 2 else "101")] = Run((15, 13) if _nz % 2 else (101,), "rocfft", nz=_nz)


def _x_variants(family, srcs):
    out = {}
    for (rows, logm), run in (((8, -1), "fused_32x16x16"), ((8, 8), "fused_512x16x16"), ((4, -1), "fused_1024x16x16")):
        for s in srcs:
            key = (family, ((s,) if s is not None else ()) + (rows, 256, logm))
            out[key] = run + ("_rot" if s == 3 else "")
    return out


CASES = {
    # ---- fused pipeline
    **_x_variants("ff_x_fwd2_kernel", (0, 1, 2, 3)),
    **_x_variants("ff_x_inv2_kernel", (None,)),
    ("ff_axis2_kernel", (0, 3, 512, -1)): "fused_32x16x16",
    ("ff_axis2_kernel", (1, 3, 512, -1)): "fused_32x16x16",
    ("ff_axis2_kernel", (2, 3, 512, -1)): "fused_32x1024x16",      # beside the 4-column y tiles
    ("ff_axis2_kernel", (0, 2, 256, -1)): "fused_32x1024x16",
    ("ff_axis2_kernel", (1, 2, 256, -1)): "fused_32x1024x16",
    ("ff_axis2_kernel", (2, 2, 256, -1)): "fused_32x16x1024",
    ("ff_axis2_fast_kernel", (0, 3, 512, 9)): "fused_32x512x16",
    ("ff_axis2_fast_kernel", (1, 3, 512, 9)): "fused_32x512x16",
    ("ff_axis2_fast_kernel", (2, 3, 512, 9)): "fused_32x16x512",
    ("ff_tile_fh2_kernel", (2,)): "fused_32x16x1024",
    ("ff_tile_fh2_kernel", (3,)): "fused_32x16x16",
    ("ff_amp_kernel", ()): "fused_32x16x16",
    # ---- generic pipeline
    ("gen_x_fwd_kernel", (0, "false")): "gen_100x100",
    ("gen_x_fwd_kernel", (1, "false")): "gen_100x100",
    ("gen_x_fwd_kernel", (2, "false")): "gen_100x100",
    ("gen_x_fwd_kernel", (3, "false")): "gen_100x100_rot",
    ("gen_x_fwd_kernel", (0, "true")): "gen_4096x16",
    ("gen_x_fwd_kernel", (1, "true")): "gen_4096x16",
    ("gen_x_fwd_kernel", (2, "true")): "gen_4096x16",
    ("gen_x_fwd_kernel", (3, "true")): "gen_4096x16_rot",
    ("gen_x_inv_kernel", ("false",)): "gen_100x100",
    ("gen_x_inv_kernel", ("true",)): "gen_4096",
    ("gen_axis_kernel", (0, 2)): "gen_20x18x600",
    ("gen_axis_kernel", (0, 3)): "gen_100x100",
    ("gen_axis_kernel", (1, 2)): "gen_20x600x18",
    ("gen_axis_kernel", (1, 3)): "gen_20x18x600",
    ("gen_axis_kernel", (2, 2)): "gen_20x18x600",
    ("gen_axis_kernel", (2, 3)): "gen_20x600x18",
    ("gen_long_outer_kernel", ("false",)): "gen_64x2048",
    ("gen_long_outer_kernel", ("true",)): "gen_64x2048",
    ("gen_long_inner_kernel", (0,)): "gen_64x2048",
    ("gen_long_inner_kernel", (2,)): "gen_64x2048",
    ("gen_tile_fh_kernel", (2,)): "gen_20x18x600",
    ("gen_tile_fh_kernel", (3,)): "gen_20x600x18",
    ("gen_tile_fh_long_kernel", ()): "gen_64x2048",
    ("gen_amp_kernel", ()): "gen_100x100",
    ("gen_phase1d_kernel", ()): "gen_4096",
    # ---- rocFFT pipeline and the shared kernels
    ("fftgs_cov_kernel", ()): "rocfft_15x13x11",
    ("fftgs_cov_rot_kernel", ()): "rocfft_15x13x11_rot",
    ("fftgs_amp_kernel", ()): "rocfft_15x13x11",
    ("fftgs_phase_kernel", ()): "rocfft_15x13x11",
    ("fftgs_scale_kernel", ()): "rocfft_15x13x11",
    ("fftgs_apply_scale_kernel", ()): "rocfft_15x13x11",
    ("fftgs_expand_kernel", ()): "rocfft_15x13x11",
    # ---- co-simulation
    **{("fftgs_lmc_mix_kernel", (nz, 2)): "lmc%d_24x20" % nz for nz in range(1, 9)},
    **{("fftgs_lmc_mix_kernel", (nz, 1)): "lmc%d_%s" % (nz, "15x13" if nz % 2 else "101") for nz in range(1, 9)},
}
