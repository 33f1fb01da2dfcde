// What the FFTGS pipelines share below the handle: the plain structs that the handle keeps and the kernels take by
// value, and the device helpers that both fftgs_fused.h and fftgs_generic.h use.  No kernel is defined here, so every
// FFTGS translation unit may include it; the kernel headers are each included by one .hip file only (the library is
// built without relocatable device code: a kernel named in two files would be compiled into both).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gss {

// source of the real input of P1
enum { FF_SRC_PHILOX = 0,   // uniform noise generated in registers (fft.jl:163 `rand(rng, V, dims)`)
       FF_SRC_ARRAY = 1,    // caller-supplied noise
       FF_SRC_COV = 2,      // covariance to the centre cell (fft.jl:96-99): the spectrum build runs on the same passes
       FF_SRC_COV_ROT = 3 };  // the same for a rotated variogram: lag := R^T lag, `noise` carries R (row-major 3 x 3)

// ---- fused pipeline (fftgs_fused.h) ----------------------------------------------------------------------------------
struct FusedGrid {
  int n1, n2, n3;      // n1 fastest; all powers of two
  int l1, l2, l3;      // log2
  int nh;              // n1 / 2 + 1
  int nhp;             // row pitch of the half-spectrum buffer: nh rounded up to FF_PITCH_ALIGN
  int ntx;             // nhp / FF_TX
  int slab_t0, slab_nt;  // strided passes restricted to the x tiles slab_t0 .. slab_t0 + slab_nt - 1 (slab_nt = 0: all)
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }

template <bool INV>
__device__ __forceinline__ double2 mul_mi(double2 a) {   // forward: a * (-i); inverse: a * (+i)
  return INV ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x);
}

template <bool INV>
__device__ __forceinline__ void x_dft4(double2& a0, double2& a1, double2& a2, double2& a3) {
  const double2 s0 = make_double2(a0.x + a2.x, a0.y + a2.y), s1 = make_double2(a0.x - a2.x, a0.y - a2.y);
  const double2 s2 = make_double2(a1.x + a3.x, a1.y + a3.y);
  const double2 s3 = mul_mi<INV>(make_double2(a1.x - a3.x, a1.y - a3.y));
  a0 = make_double2(s0.x + s2.x, s0.y + s2.y);
  a2 = make_double2(s0.x - s2.x, s0.y - s2.y);
  a1 = make_double2(s1.x + s3.x, s1.y + s3.y);
  a3 = make_double2(s1.x - s3.x, s1.y - s3.y);
}

// v <- DFT_R(v), R = 2^NS, outputs in natural order
template <int NS, bool INV>
__device__ __forceinline__ void x_dft(double2 (&v)[1 << NS]) {
  if (NS == 1) {
    const double2 a = v[0], b = v[1];
    v[0] = make_double2(a.x + b.x, a.y + b.y);
    v[1] = make_double2(a.x - b.x, a.y - b.y);
  } else if (NS == 2) {
    x_dft4<INV>(v[0], v[1], v[2], v[3]);
  } else {
    const double h = 0.70710678118654752440;
    double2 t0 = make_double2(v[0].x + v[4].x, v[0].y + v[4].y), u0 = make_double2(v[0].x - v[4].x, v[0].y - v[4].y);
    double2 t1 = make_double2(v[1].x + v[5].x, v[1].y + v[5].y), u1 = make_double2(v[1].x - v[5].x, v[1].y - v[5].y);
    double2 t2 = make_double2(v[2].x + v[6].x, v[2].y + v[6].y), u2 = make_double2(v[2].x - v[6].x, v[2].y - v[6].y);
    double2 t3 = make_double2(v[3].x + v[7].x, v[3].y + v[7].y), u3 = make_double2(v[3].x - v[7].x, v[3].y - v[7].y);
    // u_q *= W8^q (forward: exp(-i pi q / 4); inverse: conjugate)
    if (INV) {
      u1 = make_double2((u1.x - u1.y) * h, (u1.x + u1.y) * h);
      u3 = make_double2((-u3.x - u3.y) * h, (u3.x - u3.y) * h);
    } else {
      u1 = make_double2((u1.x + u1.y) * h, (u1.y - u1.x) * h);
      u3 = make_double2((u3.y - u3.x) * h, (-u3.x - u3.y) * h);
    }
    u2 = mul_mi<INV>(u2);
    x_dft4<INV>(t0, t1, t2, t3);   // -> V0, V2, V4, V6
    x_dft4<INV>(u0, u1, u2, u3);   // -> V1, V3, V5, V7
    v[0] = t0; v[2] = t1; v[4] = t2; v[6] = t3;
    v[1] = u0; v[3] = u1; v[5] = u2; v[7] = u3;
  }
}

// ---- generic pipeline (fftgs_generic.h) ------------------------------------------------------------------------------
constexpr int GEN_MAX_PASSES = 12;
struct GenPlan {          // one axis: radices of the Stockham passes and where each pass's twiddles start in its table
  int L;                  // line length (x: n1 / 2)
  int npass;
  int radix[GEN_MAX_PASSES];
  int toff[GEN_MAX_PASSES];
  int tlen;               // complex entries of the table: sum over the passes of (R - 1) * Ns
  int has7;               // a radix-7 pass: tiles of this line hold at most 7 elements per thread (g_pass)
};
struct GenGrid {
  int n1, n2, n3;         // n1 fastest; n3 = 1 on 2-D grids
  int nh, nhp;            // n1 / 2 + 1 and the row pitch of the half-spectrum buffer (a multiple of 8)
  int ndim;
  int c1, c2, c3;         // centre cell (covariance source)
  double s1, s2, s3;
};
struct GenLong {   // long y lines of a 2-D grid, split n2 = L1 * L2 (fftgs_generic.h, long lines)
  int L1, L2;      // n2 = L1 * L2
  int NB;          // values of b per outer tile (divides L2; TX * L1 * NB <= 4 096)
  int NC;          // values of c per inner tile (divides L1; TX * L2 * NC <= 4 096)
};

// ---- co-simulation (fftgs_lmc.h) -------------------------------------------------------------------------------------
constexpr int LMC_MAXZ = 8;   // the limit of gss_variogram_cross and gss_cokrig_create

// What the mixing kernel reads per cell besides the fields.  Passed by value: the coefficients are scalar operands of
// the multiplies, not loads from HBM.
struct LmcCoef {
  double L0[LMC_MAXZ * LMC_MAXZ];   // lower factor of (b0 + b0^T) / 2, row-major with stride LMC_MAXZ
  double L1[LMC_MAXZ * LMC_MAXZ];   // ... of (b1 + b1^T) / 2
  double means[LMC_MAXZ];
  uint32_t live0, live1;            // bit j: column j of the factor is not a zero column
};

}  // namespace gss
