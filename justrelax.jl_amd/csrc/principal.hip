// principal.hip -- principal stresses of the cell-centred stress tensor (compute_principal_stresses!), for gfx950.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/stokes/PrincipalStresses.jl:1-12 (compute_principal_stresses[!]), :14-40 (2D closed form),
// :42-63 (3D: hessenberg_eigen_3x3, :67-97), arrays src/types/constructors/stokes.jl:121-147 (PrincipalStress); the AMDGPU methods
// src/ext/AMDGPU/2D.jl:182-197, 3D.jl:187-202.  The operands are @stress_center(stokes) (src/Utils.jl:346-355): 2D xx, yy, xy_c; 3D xx, yy, zz, yz_c,
// xz_c, xy_c.  Outputs are (ndim, ni...) arrays, the component index fastest (Julia's σ.σ1[i, I...]).
//
// 2D: the reference's closed form as written, operation for operation (kept quirks, include/jrx.h): b = √((τxx − τyy)²/2 + τxy²), θ = atan(2τxy / (τxx − τyy)) / 2
//   with the one-argument atan, σ1 = (a + b)(cosθ, sinθ), σ2 = (a − b)(−sinθ, cosθ); 0/0 cells give NaN vectors.  σ3 (the (2, 1, 1) placeholder) is never written.
// 3D: the exact eigendecomposition (a deliberate deviation: the reference's shifted QR cannot split ±s of a simple shear and returns zeros there).
//   Cyclic Jacobi in registers with Rutishauser's rotations (the smaller root t, a_pp − t·a_pq, a_qq + t·a_pq; c = 1/√(1 + t²), s = t c), on the
//   tensor scaled by a power of two (exact) so that no square over- or underflows; a sweep starts only while the off-diagonal mass exceeds
//   (ε‖τ‖_F)², and at most kMaxSweeps sweeps run, so a NaN or Inf cell ends.  Column j of the result is λ_j e_j with λ1 ≥ λ2 ≥ λ3 and e_j a unit vector
//   whose largest-magnitude component is positive (the lowest index on ties).  A zero tensor gives zeros.
// One thread per cell, x fastest across the lanes; per cell 2D reads 24 B and writes 32 B, 3D reads 48 B and writes 72 B (three 8-B writes per output
// array at a 24-B stride: the three of a wave cover 1,536 contiguous bytes).
// The library builds with -ffp-contract=off: fma() appears only where written, so the 2D form keeps the reference's roundings.
#include "op_args.hpp"

#include <cfloat>

namespace {

constexpr int kMaxSweeps = 12;       // 3x3 cyclic Jacobi meets the exit test within a few sweeps on scaled input; the cap only ends NaN / Inf cells

// PrincipalStresses.jl:14-40
__global__ __launch_bounds__(256) void k_principal2d(double *__restrict__ s1, double *__restrict__ s2, const double *__restrict__ xx,
                                                     const double *__restrict__ yy, const double *__restrict__ xy, i64 n)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double t11 = xx[c], t22 = yy[c], t12 = xy[c];
    const double a = (t11 + t22) / 2;
    const double d = t11 - t22;
    const double b = sqrt(d * d / 2 + t12 * t12);
    const double l1 = a + b, l2 = a - b;
    const double th = atan(2 * t12 / d) / 2;
    const double sn = sin(th), cs = cos(th);
    s1[2 * c] = l1 * cs;
    s1[2 * c + 1] = l1 * sn;
    s2[2 * c] = l2 * -sn;
    s2[2 * c + 1] = l2 * cs;
}

// one Rutishauser rotation of the pair (P, Q); r is the third index, arp = a_rP, arq = a_rQ; v row-major, its columns the eigenvectors
template <int P, int Q>
__device__ __forceinline__ void rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double (&v)[9])
{
    if (!(fabs(apq) > 1e-150)) return;        // |a_pq| ≤ 1e-150 of the scaled tensor's largest entry: nothing to rotate (a NaN stays as it is)
    // t = tan φ, the smaller root of t² + 2θt − 1 = 0 with θ = (a_qq − a_pp) / (2 a_pq), written as sgn(x)·y / (|x| + √(x² + y²)) with x = a_qq − a_pp,
    // y = 2 a_pq: one division, and no overflow for entries of the scaled tensor
    const double x = aqq - app, y = 2 * apq;
    const double t = copysign(1.0, x) * y / (fabs(x) + sqrt(fma(x, x, y * y)));
    const double c = rsqrt(fma(t, t, 1.0));
    const double s = t * c;
    const double h = t * apq;
    app -= h;
    aqq += h;
    apq = 0.0;
    // the other entries and the eigenvectors: (c g − s k, s g + c k), the same rotation as Rutishauser's g − s (k + τ g), k + s (g − τ k) with
    // τ = s / (1 + c), without the division
    double g = arp, k = arq;
    arp = fma(c, g, -(s * k));
    arq = fma(s, g, c * k);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        g = v[3 * r + P];
        k = v[3 * r + Q];
        v[3 * r + P] = fma(c, g, -(s * k));
        v[3 * r + Q] = fma(s, g, c * k);
    }
}

template <int I, int J>
__device__ __forceinline__ void swap_pair(double (&l)[3], double (&v)[9])
{
    const double t = l[I];
    l[I] = l[J];
    l[J] = t;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double u = v[3 * r + I];
        v[3 * r + I] = v[3 * r + J];
        v[3 * r + J] = u;
    }
}

// PrincipalStresses.jl:42-63 with the exact eigendecomposition in place of hessenberg_eigen_3x3 (:67-97)
__global__ __launch_bounds__(256) void k_principal3d(double *__restrict__ s1, double *__restrict__ s2, double *__restrict__ s3,
                                                     const double *__restrict__ xx, const double *__restrict__ yy, const double *__restrict__ zz,
                                                     const double *__restrict__ yz, const double *__restrict__ xz, const double *__restrict__ xy, i64 n)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    double a00 = xx[c], a11 = yy[c], a22 = zz[c], a12 = yz[c], a02 = xz[c], a01 = xy[c];
    // scale by 2^-e, e the exponent of the largest |entry| (exact; skipped for a zero or non-finite tensor)
    const double m = fmax(fmax(fmax(fabs(a00), fabs(a11)), fmax(fabs(a22), fabs(a12))), fmax(fabs(a02), fabs(a01)));
    int e = 0;
    if (m > 0.0 && m <= DBL_MAX) {
        e = max(ilogb(m), -1020);
        const double sc = ldexp(1.0, -e);
        a00 *= sc; a11 *= sc; a22 *= sc; a12 *= sc; a02 *= sc; a01 *= sc;
    }
    double v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    const double off0 = a01 * a01 + a02 * a02 + a12 * a12;
    const double tol2 = DBL_EPSILON * DBL_EPSILON * (a00 * a00 + a11 * a11 + a22 * a22 + 2 * off0);      // (ε‖τ‖_F)²
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        const double off = 2 * (a01 * a01 + a02 * a02 + a12 * a12);
        if (!(off > tol2)) break;
        rotate<0, 1>(a00, a11, a01, a02, a12, v);
        rotate<0, 2>(a00, a22, a02, a01, a12, v);
        rotate<1, 2>(a11, a22, a12, a01, a02, v);
    }
    // descending order (a fixed network: deterministic on ties), then the sign rule, then λ_j e_j at the caller's scale
    double l[3] = {a00, a11, a22};
    if (l[0] < l[1]) swap_pair<0, 1>(l, v);
    if (l[1] < l[2]) swap_pair<1, 2>(l, v);
    if (l[0] < l[1]) swap_pair<0, 1>(l, v);
    double *out[3] = {s1, s2, s3};
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double e0 = v[j], e1 = v[3 + j], e2 = v[6 + j];
        double big = e0;
        if (fabs(e1) > fabs(big)) big = e1;
        if (fabs(e2) > fabs(big)) big = e2;
        const double lam = ldexp(big < 0.0 ? -l[j] : l[j], e);
        out[j][3 * c] = lam * e0;
        out[j][3 * c + 1] = lam * e1;
        out[j][3 * c + 2] = lam * e2;
    }
}

// both entry points: s the ND outputs σ1 .. σND (ND values per cell), t the components of the stress (3 in 2D, 6 in 3D)
jrx_status ps_compute(jrx_handle *h, int ND, double *const *s, const double *const *t, const int64_t n[3])
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "compute_principal_stresses!";
    const int NT = ND == 2 ? 3 : 6;
    bool null = false;
    for (int a = 0; a < ND; a++) null = null || !s[a];
    for (int q = 0; q < NT; q++) null = null || !t[q];
    if (null) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (!op_extents_ok(n, ND)) return jrx_fail(h, JRX_ERR_ARG, "%s: size(stokes.P) = (%s)", fn, op_list(n, ND, ", ").s);
    if (op_count(n, ND, 0) >= 2147483648.0 * 256.0) return jrx_fail(h, JRX_ERR_UNSUPPORTED, "%s: 2^39 or more cells", fn);      // 64-bit offsets; 2^31 blocks of 256
    const i64 bytes = op_bytes(n, ND, 0, 0, 0), cells = bytes / 8;
    OpArr out[3], in[6];
    for (int a = 0; a < ND; a++) out[a] = OpArr{s[a], ND * bytes, nullptr};
    for (int q = 0; q < NT; q++) in[q] = OpArr{t[q], bytes, nullptr};
    if (const OpClash c = op_disjoint(out, ND, in, NT))
        return c.two ? jrx_fail(h, JRX_ERR_ARG, "%s: σ%d and σ%d overlap", fn, c.a + 1, c.b + 1)
                     : jrx_fail(h, JRX_ERR_ARG, "%s: an output overlaps a stress component", fn);
    JRX_TRY(jrx_check_device(h));
    h->stat_principal_calls++;
    const dim3 grid((unsigned)((cells + 255) / 256)), block(256);
    if (ND == 2) hipLaunchKernelGGL(k_principal2d, grid, block, 0, h->stream, s[0], s[1], t[0], t[1], t[2], cells);
    else hipLaunchKernelGGL(k_principal3d, grid, block, 0, h->stream, s[0], s[1], s[2], t[0], t[1], t[2], t[3], t[4], t[5], cells);
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_principal_stresses2d(jrx_handle *h, double *s1, double *s2, const double *xx, const double *yy, const double *xy_c, int64_t nx, int64_t ny)
{
    double *const s[2] = {s1, s2};
    const double *const t[3] = {xx, yy, xy_c};
    const int64_t n[3] = {nx, ny, 1};
    return ps_compute(h, 2, s, t, n);
}

jrx_status jrx_principal_stresses3d(jrx_handle *h, double *s1, double *s2, double *s3, const double *xx, const double *yy, const double *zz,
                                    const double *yz_c, const double *xz_c, const double *xy_c, int64_t nx, int64_t ny, int64_t nz)
{
    double *const s[3] = {s1, s2, s3};
    const double *const t[6] = {xx, yy, zz, yz_c, xz_c, xy_c};
    const int64_t n[3] = {nx, ny, nz};
    return ps_compute(h, 3, s, t, n);
}

}  // extern "C"
