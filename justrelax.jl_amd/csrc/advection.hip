// advection.hip -- WENO-5 advection of a 2D or 3D vertex field (WENO_advection!), for gfx950.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/advection/weno5.jl:10-16 (betas), :23-55 (alphas, Val(1) JS / Val(2) Z), :59-71 (candidate
// stencils), :84-107 (weights and flux), :120-151 (clamped stencils), :154-168 (weno_rhs), :170-175 (weno_f!), :195-230 (WENO_advection!: SSP-RK3 as six
// @parallel launches); constants src/types/constructors/weno.jl:7-24; the AMDGPU methods src/ext/AMDGPU/2D.jl:84-88,470-472.
//
// Two forms built from the same __device__ functions below, so u and ut come out bit-identical:
//   per-kernel (the reference's shape, tuning "weno_fused" = 0): k_weno_flux writes fL, fR, fB, fT, k_weno_step<S> reads them; three times = six launches.
//   fused (default): one launch per RK stage; every flux lives in registers and is computed once.  A wave owns 64 consecutive x columns (62 outputs, one
//     flux column either side) and marches in y over a chunk of rows: the five-row y window of the field is in registers, the y fluxes run one row ahead,
//     the x stencil and the x-neighbour fluxes come from the neighbouring lanes (__shfl); the two lanes at either end load the two columns beyond the wave.
//     Stage 1 reads the stencil of u and writes u1 into fL (the reference's own allocation: nothing outside weno5.jl reads fL..fT), stage 2 reads the
//     stencil of u1 plus u at the point and writes ut, stage 3 reads the stencil of ut plus u at the point and writes u in place (it reads u only at its
//     own vertex).  No stage writes the array whose neighbours it reads.
// Upwind and downwind flux of a direction share the betas and inv(β + ϵ) (same operations on the same operands: the bits do not change).
// fma() stands where the reference has muladd / @muladd; the library builds with -ffp-contract=off, so nothing else is contracted.
// 3D (jrx_weno5_advection3d): the scheme is defined one direction at a time, so its 3D form is the same clamped five-point reconstruction along z (fD upwind,
// fU downwind: this project's names), two more terms in weno_rhs and the same SSP-RK3 -- the reference's own 3D methods (src/ext/AMDGPU/3D.jl:71-75,493-495)
// feed a 3D array into the 2D indexing of weno5.jl.  Again two forms from the same __device__ functions:
//   per-kernel: k_weno_flux3d writes the six fluxes, k_weno_step3d<S> reads them; six launches.
//   fused: one launch per RK stage.  A block is 64 columns x 8 rows of vertices (62 x 6 outputs, one flux column / row either side) and marches in z over a
//     chunk of planes: every thread keeps the five-plane z window of its vertex in registers with the z fluxes one plane ahead (the 2D kernel's y march), takes
//     the x stencil and the x-neighbour fluxes from the neighbouring lanes, and the y stencil and the y-neighbour fluxes of the current plane from LDS (two
//     block barriers per plane).  The first and last wave of a block are the y halo: they evaluate only the y fluxes of their row.
// Addressing: 32-bit element offsets (every array below 2^31 entries, checked).
#include "op_args.hpp"

namespace {

// constructors/weno.jl:7-24
constexpr double kD0L = 1.0 / 10, kD1L = 3.0 / 5, kD2L = 3.0 / 10;
constexpr double kD0R = 3.0 / 10, kD1R = 3.0 / 5, kD2R = 1.0 / 10;
constexpr double kC1 = 13.0 / 12, kC2 = 1.0 / 4;
constexpr double kSc1 = 1.0 / 3, kSc2 = 7.0 / 6, kSc3 = 11.0 / 6, kSc4 = 1.0 / 6, kSc5 = 5.0 / 6;
constexpr double kEps = 1.0e-6;

// The upwind (fup: fB / fL) and downwind (fdn: fT / fR) flux of one direction from the five clamped values u[i-2..i+2] -- _WENO_u (weno5.jl:84-107) twice,
// with the betas (:10-16) and inv(β + ϵ) shared.  M = 1: JS alphas d inv(β + ϵ)^2; M = 2: Z alphas d (1 + (τ inv(β + ϵ))^2), τ = |β0 - β2|.
template <int M>
__device__ __forceinline__ void weno_pair(double u1, double u2, double u3, double u4, double u5, double &fup, double &fdn)
{
    const double a0 = fma(-2.0, u2, u1) + u3, b0 = fma(3.0, u3, fma(-4.0, u2, u1));
    const double a1 = fma(-2.0, u3, u2) + u4, b1 = u2 - u4;
    const double a2 = fma(-2.0, u4, u3) + u5, b2 = fma(-4.0, u4, 3.0 * u3) + u5;
    const double be0 = fma(kC1, a0 * a0, kC2 * (b0 * b0));
    const double be1 = fma(kC1, a1 * a1, kC2 * (b1 * b1));
    const double be2 = fma(kC1, a2 * a2, kC2 * (b2 * b2));
    const double q0 = 1.0 / (be0 + kEps), q1 = 1.0 / (be1 + kEps), q2 = 1.0 / (be2 + kEps);
    double g0, g1, g2;
    if (M == 1) {
        g0 = q0 * q0; g1 = q1 * q1; g2 = q2 * q2;
    } else {
        const double tau = fabs(be0 - be2), t0 = tau * q0, t1 = tau * q1, t2 = tau * q2;
        g0 = 1.0 + t0 * t0; g1 = 1.0 + t1 * t1; g2 = 1.0 + t2 * t2;
    }
    {   // upwind: weno_alphas_upwind (:23-38), stencil_candidate_upwind (:59-64)
        const double al0 = kD0L * g0, al1 = kD1L * g1, al2 = kD2L * g2;
        const double _a = 1.0 / (al0 + al1 + al2);
        const double w0 = al0 * _a, w1 = al1 * _a, w2 = al2 * _a;
        const double s0 = fma(kSc3, u3, fma(-kSc2, u2, kSc1 * u1));
        const double s1 = fma(kSc1, u4, fma(kSc5, u3, -kSc4 * u2));
        const double s2 = fma(-kSc4, u5, fma(kSc5, u4, kSc1 * u3));
        fup = fma(w0, s0, fma(w1, s1, w2 * s2));
    }
    {   // downwind: weno_alphas_downwind (:40-55), stencil_candidate_downwind (:66-71)
        const double al0 = kD0R * g0, al1 = kD1R * g1, al2 = kD2R * g2;
        const double _a = 1.0 / (al0 + al1 + al2);
        const double w0 = al0 * _a, w1 = al1 * _a, w2 = al2 * _a;
        const double s0 = fma(kSc1, u3, fma(kSc5, u2, -kSc4 * u1));
        const double s1 = fma(-kSc4, u4, fma(kSc5, u3, kSc1 * u2));
        const double s2 = fma(kSc1, u5, fma(-kSc2, u4, kSc3 * u3));
        fdn = fma(w0, s0, fma(w1, s1, w2 * s2));
    }
}

// weno_rhs (weno5.jl:154-168).  fBS = fB[iS], fTN = fT[iN], fLW = fL[jW], fRE = fR[jE] with clamped iS, iN, jW, jE: at the first / last vertex of a direction
// the caller passes the flux itself, and that difference is exactly 0 (the reference's quirk, kept)
__device__ __forceinline__ double weno_rhs(double vx, double vy, double fB, double fBS, double fT, double fTN, double fL, double fLW, double fR, double fRE,
                                           double _dx, double _dy)
{
    double r = (fmin(vy, 0.0) * (fRE - fR)) * _dy;
    r = fma(fmax(vy, 0.0) * (fL - fLW), _dy, r);
    r = fma(fmin(vx, 0.0) * (fTN - fT), _dx, r);
    return fma(fmax(vx, 0.0) * (fB - fBS), _dx, r);
}

// weno_rhs one dimension up: the two z terms innermost (fDD = fD[kD], fUU = fU[kU], clamped like the others), then the y and x chain of weno_rhs in its order.
// With a field constant along z both z terms are exactly 0 and the result has the bits of weno_rhs.
__device__ __forceinline__ double weno_rhs3(double vx, double vy, double vz, double fB, double fBS, double fT, double fTN, double fL, double fLW, double fR,
                                            double fRE, double fD, double fDD, double fU, double fUU, double _dx, double _dy, double _dz)
{
    double r = (fmin(vz, 0.0) * (fUU - fU)) * _dz;
    r = fma(fmax(vz, 0.0) * (fD - fDD), _dz, r);
    r = fma(fmin(vy, 0.0) * (fRE - fR), _dy, r);
    r = fma(fmax(vy, 0.0) * (fL - fLW), _dy, r);
    r = fma(fmin(vx, 0.0) * (fTN - fT), _dx, r);
    return fma(fmax(vx, 0.0) * (fB - fBS), _dx, r);
}

// weno_step1! / 2! / 3! (weno5.jl:210-230): u = the field at the start of the call, ut = the previous stage's field (stages 2, 3)
template <int S>
__device__ __forceinline__ double weno_stage(double u, double ut, double r, double dt)
{
    if (S == 1) return fma(-dt, r, u);
    if (S == 2) return fma(0.75, u, fma(0.25, ut, -(0.25 * dt) * r));
    constexpr double one_third = 1.0 / 3, two_thirds = 2 * one_third;
    return fma(one_third, u, fma(two_thirds, ut, -(two_thirds * dt) * r));
}

// ---------------------------------------------------------------- per-kernel form
// weno_f! (weno5.jl:170-175) over the (nx, ny) box of u: src has leading extent ls, the flux arrays lw
template <int M>
__global__ __launch_bounds__(256) void k_weno_flux(double *__restrict__ fL, double *__restrict__ fR, double *__restrict__ fB, double *__restrict__ fT,
                                                   const double *__restrict__ src, int nx, int ny, int ls, int lw)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x, j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const double *row = src + ls * j;
    double fb, ft, fl, fr;
    weno_pair<M>(row[clampi(i - 2, 0, nx - 1)], row[clampi(i - 1, 0, nx - 1)], row[i], row[clampi(i + 1, 0, nx - 1)], row[clampi(i + 2, 0, nx - 1)], fb, ft);
    weno_pair<M>(src[i + ls * clampi(j - 2, 0, ny - 1)], src[i + ls * clampi(j - 1, 0, ny - 1)], row[i], src[i + ls * clampi(j + 1, 0, ny - 1)],
                 src[i + ls * clampi(j + 2, 0, ny - 1)], fl, fr);
    const int o = i + lw * j;
    fB[o] = fb; fT[o] = ft; fL[o] = fl; fR[o] = fr;
}

// weno_step<S>! with weno_rhs from the flux arrays.  S = 1, 2 write ut; S = 3 writes u (it reads u only at its own vertex, hence no __restrict__ on u / ut)
template <int S>
__global__ __launch_bounds__(256) void k_weno_step(double *u, double *ut, const double *__restrict__ fL, const double *__restrict__ fR,
                                                   const double *__restrict__ fB, const double *__restrict__ fT, const double *__restrict__ vx,
                                                   const double *__restrict__ vy, int nx, int ny, int lu, int lw, int lvx, int lvy, double _dx, double _dy, double dt)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x, j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const int o = i + lw * j;
    const int iS = clampi(i - 1, 0, nx - 1), iN = clampi(i + 1, 0, nx - 1), jW = clampi(j - 1, 0, ny - 1), jE = clampi(j + 1, 0, ny - 1);
    const double r = weno_rhs(vx[i + lvx * j], vy[i + lvy * j], fB[o], fB[iS + lw * j], fT[o], fT[iN + lw * j], fL[o], fL[i + lw * jW], fR[o], fR[i + lw * jE],
                              _dx, _dy);
    const double un = weno_stage<S>(u[i + lu * j], S == 1 ? 0.0 : ut[o], r, dt);
    if (S == 3) u[i + lu * j] = un;
    else ut[o] = un;
}

// ---------------------------------------------------------------- fused form
constexpr int kWenoLanes = 64, kWenoOut = 62, kWenoWaves = 4;     // a wave: 64 columns, 62 outputs; four independent waves per block, stacked in y

// One RK stage.  src: the stencil field (leading extent ls; u, u1 or ut), dst: the output (ld), u0: u at the point (lu; stages 2, 3 -- stage 3 writes
// dst = u0 in place).  Wave (blockIdx.x, w) covers columns 62 bx - 1 .. 62 bx + 62 and rows [rows (4 by + w), + rows).
template <int M, int S>
__global__ __launch_bounds__(256) void k_weno_fused(double *dst, const double *__restrict__ src, const double *u0, const double *__restrict__ vx,
                                                    const double *__restrict__ vy, int nx, int ny, int ls, int ld, int lu, int lvx, int lvy, int rows,
                                                    double _dx, double _dy, double dt)
{
    const int lane = threadIdx.x;
    const int j0 = (blockIdx.y * kWenoWaves + threadIdx.y) * rows;
    if (j0 >= ny) return;                                         // uniform over the wave
    const int j1 = min(j0 + rows, ny);
    const int c = blockIdx.x * kWenoOut - 1 + lane;              // this lane's column (may lie outside 0 .. nx-1: clamped loads, no store)
    const int cc = clampi(c, 0, nx - 1);
    const bool edge = lane < 2 || lane >= kWenoLanes - 2;
    const int ce = clampi(lane < 2 ? c - 2 : c + 2, 0, nx - 1);  // the column beyond the wave an end lane holds
    const bool out = lane >= 1 && lane <= kWenoOut && c < nx;
    const int ym = ny - 1;
    auto at = [&](int col, int row) { return src[col + ls * clampi(row, 0, ym)]; };

    // y window: rows j0-2 .. j0+2 after the prologue; the y fluxes of rows j0-1 (fL) and j0 (fL, fR)
    const double w0 = at(cc, j0 - 3);
    double a0 = at(cc, j0 - 2), a1 = at(cc, j0 - 1), a2 = at(cc, j0), a3 = at(cc, j0 + 1), a4 = at(cc, j0 + 2);
    double fLm, fLc, fRc, dummy;
    weno_pair<M>(w0, a0, a1, a2, a3, fLm, dummy);
    weno_pair<M>(a0, a1, a2, a3, a4, fLc, fRc);
    double nxt = at(cc, j0 + 3);
    double en = edge ? at(ce, j0) : 0.0;
    for (int j = j0; j < j1; j++) {
        const double a5 = nxt, ec = en;
        nxt = at(cc, j + 4);                                      // one row ahead
        en = edge ? at(ce, j + 1) : 0.0;
        const double vxv = vx[cc + lvx * j], vyv = vy[cc + lvy * j];
        const double uv = S == 1 ? a2 : u0[cc + lu * j];
        // x fluxes of row j at this lane's column: the stencil from the lanes either side (the end lanes' extra columns for the lanes next to the ends)
        const double sm2 = __shfl(a2, lane - 2, 64), sm1 = __shfl(a2, lane - 1, 64), sp1 = __shfl(a2, lane + 1, 64), sp2 = __shfl(a2, lane + 2, 64);
        const double e1 = __shfl(ec, 1, 64), e62 = __shfl(ec, kWenoLanes - 2, 64);
        const double um2 = lane >= 2 ? sm2 : ec, um1 = lane >= 1 ? sm1 : e1;
        const double up1 = lane <= kWenoLanes - 2 ? sp1 : e62, up2 = lane <= kWenoLanes - 3 ? sp2 : ec;
        double fB, fT;
        weno_pair<M>(um2, um1, a2, up1, up2, fB, fT);
        const double fBl = __shfl(fB, lane - 1, 64), fTr = __shfl(fT, lane + 1, 64);
        // y fluxes of row j + 1
        double fLn, fRn;
        weno_pair<M>(a1, a2, a3, a4, a5, fLn, fRn);
        const double r = weno_rhs(vxv, vyv, fB, c == 0 ? fB : fBl, fT, c == nx - 1 ? fT : fTr, fLc, j == 0 ? fLc : fLm, fRc, j == ym ? fRc : fRn, _dx, _dy);
        if (out) dst[c + ld * j] = weno_stage<S>(uv, a2, r, dt);
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5;
        fLm = fLc; fLc = fLn; fRc = fRn;
    }
    (void)a0;
}

// rows a wave marches: 64, halved (down to 8) while the launch would have fewer than 4,096 waves
int fused_rows(const jrx_handle *h, int nx, int ny)
{
    if (h->weno_rows > 0) return h->weno_rows;
    const long nbx = (nx + kWenoOut - 1) / kWenoOut;
    int rows = 64;
    while (rows > 8 && nbx * ((ny + rows - 1) / rows) < 4096) rows /= 2;
    return rows;
}

template <int M>
jrx_status launch_fused(jrx_handle *h, double *u, double *ut, double *u1, const double *vx, const double *vy, int nx, int ny, int lu, int lw, int lvx, int lvy,
                        double _dx, double _dy, double dt)
{
    const int rows = fused_rows(h, nx, ny);
    const int nchunk = (ny + rows - 1) / rows;
    const dim3 grid((unsigned)((nx + kWenoOut - 1) / kWenoOut), (unsigned)((nchunk + kWenoWaves - 1) / kWenoWaves)), block(kWenoLanes, kWenoWaves);
    hipLaunchKernelGGL((k_weno_fused<M, 1>), grid, block, 0, h->stream, u1, u, u, vx, vy, nx, ny, lu, lw, lu, lvx, lvy, rows, _dx, _dy, dt);
    hipLaunchKernelGGL((k_weno_fused<M, 2>), grid, block, 0, h->stream, ut, u1, u, vx, vy, nx, ny, lw, lw, lu, lvx, lvy, rows, _dx, _dy, dt);
    hipLaunchKernelGGL((k_weno_fused<M, 3>), grid, block, 0, h->stream, u, ut, u, vx, vy, nx, ny, lw, lu, lu, lvx, lvy, rows, _dx, _dy, dt);
    return JRX_OK;
}

template <int M>
jrx_status launch_split(jrx_handle *h, double *u, double *ut, double *fL, double *fR, double *fB, double *fT, const double *vx, const double *vy, int nx, int ny,
                        int lu, int lw, int lvx, int lvy, double _dx, double _dy, double dt)
{
    const dim3 grid((unsigned)(((int64_t)nx * ny + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_weno_flux<M>, grid, block, 0, h->stream, fL, fR, fB, fT, u, nx, ny, lu, lw);
    hipLaunchKernelGGL(k_weno_step<1>, grid, block, 0, h->stream, u, ut, fL, fR, fB, fT, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt);
    hipLaunchKernelGGL(k_weno_flux<M>, grid, block, 0, h->stream, fL, fR, fB, fT, ut, nx, ny, lw, lw);
    hipLaunchKernelGGL(k_weno_step<2>, grid, block, 0, h->stream, u, ut, fL, fR, fB, fT, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt);
    hipLaunchKernelGGL(k_weno_flux<M>, grid, block, 0, h->stream, fL, fR, fB, fT, ut, nx, ny, lw, lw);
    hipLaunchKernelGGL(k_weno_step<3>, grid, block, 0, h->stream, u, ut, fL, fR, fB, fT, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt);
    return JRX_OK;
}

// ================================================================ 3D
struct WenoExt { int ly, lz; };                                  // element strides of an array along y and z (its own extents: ly = n1, lz = n1 n2)

// ---------------------------------------------------------------- per-kernel form (3D)
template <int M>
__global__ __launch_bounds__(256) void k_weno_flux3d(double *__restrict__ fL, double *__restrict__ fR, double *__restrict__ fB, double *__restrict__ fT,
                                                     double *__restrict__ fD, double *__restrict__ fU, const double *__restrict__ src, int nx, int ny, int nz,
                                                     WenoExt es, WenoExt ew)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = (int)(t / ((int64_t)nx * ny));
    if (k >= nz) return;
    const int q = (int)(t - (int64_t)k * nx * ny), j = q / nx, i = q - j * nx;
    auto at = [&](int a, int b, int c) { return src[clampi(a, 0, nx - 1) + es.ly * clampi(b, 0, ny - 1) + es.lz * clampi(c, 0, nz - 1)]; };
    const double uc = at(i, j, k);
    double fb, ft, fl, fr, fd, fu;
    weno_pair<M>(at(i - 2, j, k), at(i - 1, j, k), uc, at(i + 1, j, k), at(i + 2, j, k), fb, ft);
    weno_pair<M>(at(i, j - 2, k), at(i, j - 1, k), uc, at(i, j + 1, k), at(i, j + 2, k), fl, fr);
    weno_pair<M>(at(i, j, k - 2), at(i, j, k - 1), uc, at(i, j, k + 1), at(i, j, k + 2), fd, fu);
    const int o = i + ew.ly * j + ew.lz * k;
    fB[o] = fb; fT[o] = ft; fL[o] = fl; fR[o] = fr; fD[o] = fd; fU[o] = fu;
}

template <int S>
__global__ __launch_bounds__(256) void k_weno_step3d(double *u, double *ut, const double *__restrict__ fL, const double *__restrict__ fR,
                                                     const double *__restrict__ fB, const double *__restrict__ fT, const double *__restrict__ fD,
                                                     const double *__restrict__ fU, const double *__restrict__ vx, const double *__restrict__ vy,
                                                     const double *__restrict__ vz, int nx, int ny, int nz, WenoExt eu, WenoExt ew, WenoExt evx, WenoExt evy,
                                                     WenoExt evz, double _dx, double _dy, double _dz, double dt)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = (int)(t / ((int64_t)nx * ny));
    if (k >= nz) return;
    const int q = (int)(t - (int64_t)k * nx * ny), j = q / nx, i = q - j * nx;
    const int o = i + ew.ly * j + ew.lz * k, ou = i + eu.ly * j + eu.lz * k;
    const int iS = clampi(i - 1, 0, nx - 1), iN = clampi(i + 1, 0, nx - 1), jW = clampi(j - 1, 0, ny - 1), jE = clampi(j + 1, 0, ny - 1);
    const int kD = clampi(k - 1, 0, nz - 1), kU = clampi(k + 1, 0, nz - 1);
    const double r = weno_rhs3(vx[i + evx.ly * j + evx.lz * k], vy[i + evy.ly * j + evy.lz * k], vz[i + evz.ly * j + evz.lz * k], fB[o],
                               fB[iS + ew.ly * j + ew.lz * k], fT[o], fT[iN + ew.ly * j + ew.lz * k], fL[o], fL[i + ew.ly * jW + ew.lz * k], fR[o],
                               fR[i + ew.ly * jE + ew.lz * k], fD[o], fD[i + ew.ly * j + ew.lz * kD], fU[o], fU[i + ew.ly * j + ew.lz * kU], _dx, _dy, _dz);
    const double un = weno_stage<S>(u[ou], S == 1 ? 0.0 : ut[o], r, dt);
    if (S == 3) u[ou] = un;
    else ut[o] = un;
}

// ---------------------------------------------------------------- fused form (3D)
constexpr int kWeno3Rows = 8, kWeno3Out = kWeno3Rows - 2;        // a block: 8 waves stacked in y (6 output rows, a y-flux row either side), 64 columns each as in 2D

// One RK stage; src / dst / u0 as in k_weno_fused.  Block (bx, by, bz) of the 1D grid covers columns 62 bx - 1 .. 62 bx + 62, rows 6 by - 1 .. 6 by + 6 and planes
// [planes bz, + planes).  Wave ty owns row 6 by - 1 + ty; waves 0 and 7 only feed the y fluxes of their row to waves 1 and 6.  Per plane: every wave puts the
// plane's value of its vertex into sv (the first and last two waves also the row two beyond), barrier, every wave forms its y flux pair from sv and puts it
// into sL / sR, barrier, the six inner waves read fL of the row below and fR of the row above.  The next plane's writes of sv come after the second barrier
// (every read of sv is before it) and its writes of sL / sR after the next first barrier (every read of sL / sR is before it): single buffers suffice.
template <int M, int S>
__global__ __launch_bounds__(64 * kWeno3Rows) void k_weno_fused3d(double *dst, const double *__restrict__ src, const double *u0, const double *__restrict__ vx,
                                                                  const double *__restrict__ vy, const double *__restrict__ vz, int nx, int ny, int nz, WenoExt es,
                                                                  WenoExt ed, WenoExt eu, WenoExt evx, WenoExt evy, WenoExt evz, int nbx, int nby, int planes, double _dx,
                                                                  double _dy, double _dz, double dt)
{
    __shared__ double sv[kWeno3Rows + 4][kWenoLanes], sL[kWeno3Rows][kWenoLanes], sR[kWeno3Rows][kWenoLanes];
    const int lane = threadIdx.x, ty = threadIdx.y;
    const int bz = blockIdx.x / (nbx * nby), bq = blockIdx.x - bz * (nbx * nby), by = bq / nbx, bx = bq - by * nbx;   // 1D grid, x fastest
    const int k0 = bz * planes, k1 = min(k0 + planes, nz);                  // uniform over the block; k0 < nz by the grid
    const int c = bx * kWenoOut - 1 + lane, cc = clampi(c, 0, nx - 1);
    const int r = by * kWeno3Out - 1 + ty, rr = clampi(r, 0, ny - 1);
    const bool inner = ty >= 1 && ty <= kWeno3Out;                           // uniform over the wave
    const bool xedge = inner && (lane < 2 || lane >= kWenoLanes - 2);
    const int ce = clampi(lane < 2 ? c - 2 : c + 2, 0, nx - 1);             // the column beyond the wave an end lane holds
    const bool yedge = ty < 2 || ty >= kWeno3Rows - 2;
    const int re = clampi(ty < 2 ? r - 2 : r + 2, 0, ny - 1);               // the row beyond the block a wave of the first / last two holds
    const int se = ty < 2 ? ty : ty + 4;                                     // ... and its row of sv
    const bool out = inner && lane >= 1 && lane <= kWenoOut && c < nx && r < ny;
    const int xm = nx - 1, ym = ny - 1, zm = nz - 1;
    auto at = [&](int col, int row, int k) { return src[col + es.ly * row + es.lz * clampi(k, 0, zm)]; };

    // z window: planes k0-2 .. k0+2 after the prologue; the z fluxes of planes k0-1 (fD) and k0 (fD, fU)
    const double w0 = at(cc, rr, k0 - 3);
    double a0 = at(cc, rr, k0 - 2), a1 = at(cc, rr, k0 - 1), a2 = at(cc, rr, k0), a3 = at(cc, rr, k0 + 1), a4 = at(cc, rr, k0 + 2);
    double fDm = 0.0, fDc = 0.0, fUc = 0.0, dummy;
    if (inner) {
        weno_pair<M>(w0, a0, a1, a2, a3, fDm, dummy);
        weno_pair<M>(a0, a1, a2, a3, a4, fDc, fUc);
    }
    double nxt = at(cc, rr, k0 + 3);
    double en = xedge ? at(ce, rr, k0) : 0.0, yn = yedge ? at(cc, re, k0) : 0.0;
    for (int k = k0; k < k1; k++) {
        const double a5 = nxt, ec = en, yc = yn;
        nxt = at(cc, rr, k + 4);                                            // one plane ahead
        en = xedge ? at(ce, rr, k + 1) : 0.0;
        yn = yedge ? at(cc, re, k + 1) : 0.0;
        double vxv = 0.0, vyv = 0.0, vzv = 0.0, uv = a2;
        if (inner) {
            vxv = vx[cc + evx.ly * rr + evx.lz * k]; vyv = vy[cc + evy.ly * rr + evy.lz * k]; vzv = vz[cc + evz.ly * rr + evz.lz * k];
            if (S != 1) uv = u0[cc + eu.ly * rr + eu.lz * k];
        }
        sv[ty + 2][lane] = a2;
        if (yedge) sv[se][lane] = yc;
        __syncthreads();
        double fL, fR;                                                      // y fluxes of this row
        weno_pair<M>(sv[ty][lane], sv[ty + 1][lane], a2, sv[ty + 3][lane], sv[ty + 4][lane], fL, fR);
        sL[ty][lane] = fL; sR[ty][lane] = fR;
        __syncthreads();
        if (inner) {
            // x fluxes, as in k_weno_fused
            const double sm2 = __shfl(a2, lane - 2, 64), sm1 = __shfl(a2, lane - 1, 64), sp1 = __shfl(a2, lane + 1, 64), sp2 = __shfl(a2, lane + 2, 64);
            const double e1 = __shfl(ec, 1, 64), e62 = __shfl(ec, kWenoLanes - 2, 64);
            const double um2 = lane >= 2 ? sm2 : ec, um1 = lane >= 1 ? sm1 : e1;
            const double up1 = lane <= kWenoLanes - 2 ? sp1 : e62, up2 = lane <= kWenoLanes - 3 ? sp2 : ec;
            double fB, fT;
            weno_pair<M>(um2, um1, a2, up1, up2, fB, fT);
            const double fBl = __shfl(fB, lane - 1, 64), fTr = __shfl(fT, lane + 1, 64);
            // z fluxes of plane k + 1
            double fDn, fUn;
            weno_pair<M>(a1, a2, a3, a4, a5, fDn, fUn);
            const double fLW = sL[ty - 1][lane], fRE = sR[ty + 1][lane];
            const double rh = weno_rhs3(vxv, vyv, vzv, fB, c == 0 ? fB : fBl, fT, c == xm ? fT : fTr, fL, r == 0 ? fL : fLW, fR, r == ym ? fR : fRE, fDc,
                                        k == 0 ? fDc : fDm, fUc, k == zm ? fUc : fUn, _dx, _dy, _dz);
            if (out) dst[c + ed.ly * r + ed.lz * k] = weno_stage<S>(uv, a2, rh, dt);
            fDm = fDc; fDc = fDn; fUc = fUn;
        }
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5;
    }
    (void)a0;
}

// planes a block marches: 64, halved (down to 8) while the launch would have fewer than 1,024 blocks (8,192 waves)
int fused_planes(const jrx_handle *h, int nx, int ny, int nz)
{
    if (h->weno_rows > 0) return h->weno_rows;
    const long nb = (long)((nx + kWenoOut - 1) / kWenoOut) * ((ny + kWeno3Out - 1) / kWeno3Out);
    int planes = 64;
    while (planes > 8 && nb * ((nz + planes - 1) / planes) < 1024) planes /= 2;
    return planes;
}

struct Weno3Args {
    double *u, *ut, *f[6];                                       // f: fL, fR, fB, fT, fD, fU
    const double *vx, *vy, *vz;
    int nx, ny, nz;
    WenoExt eu, ew, evx, evy, evz;
    double _dx, _dy, _dz, dt;
};

template <int M>
jrx_status launch_fused3d(jrx_handle *h, const Weno3Args &a)
{
    const int planes = fused_planes(h, a.nx, a.ny, a.nz);
    const int nbx = (a.nx + kWenoOut - 1) / kWenoOut, nby = (a.ny + kWeno3Out - 1) / kWeno3Out, nbz = (a.nz + planes - 1) / planes;
    const dim3 grid((unsigned)((int64_t)nbx * nby * nbz)), block(kWenoLanes, kWeno3Rows);     // below 2^31 blocks: every array is below 2^31 entries
    double *u1 = a.f[0];
    hipLaunchKernelGGL((k_weno_fused3d<M, 1>), grid, block, 0, h->stream, u1, a.u, a.u, a.vx, a.vy, a.vz, a.nx, a.ny, a.nz, a.eu, a.ew, a.eu, a.evx, a.evy, a.evz,
                       nbx, nby, planes, a._dx, a._dy, a._dz, a.dt);
    hipLaunchKernelGGL((k_weno_fused3d<M, 2>), grid, block, 0, h->stream, a.ut, u1, a.u, a.vx, a.vy, a.vz, a.nx, a.ny, a.nz, a.ew, a.ew, a.eu, a.evx, a.evy, a.evz,
                       nbx, nby, planes, a._dx, a._dy, a._dz, a.dt);
    hipLaunchKernelGGL((k_weno_fused3d<M, 3>), grid, block, 0, h->stream, a.u, a.ut, a.u, a.vx, a.vy, a.vz, a.nx, a.ny, a.nz, a.ew, a.eu, a.eu, a.evx, a.evy, a.evz,
                       nbx, nby, planes, a._dx, a._dy, a._dz, a.dt);
    return JRX_OK;
}

template <int M>
jrx_status launch_split3d(jrx_handle *h, const Weno3Args &a)
{
    const dim3 grid((unsigned)(((int64_t)a.nx * a.ny * a.nz + 255) / 256)), block(256);
    double *const *f = a.f;
    for (int s = 1; s <= 3; s++) {
        hipLaunchKernelGGL(k_weno_flux3d<M>, grid, block, 0, h->stream, f[0], f[1], f[2], f[3], f[4], f[5], s == 1 ? a.u : a.ut, a.nx, a.ny, a.nz,
                           s == 1 ? a.eu : a.ew, a.ew);
        auto step = s == 1 ? k_weno_step3d<1> : s == 2 ? k_weno_step3d<2> : k_weno_step3d<3>;
        hipLaunchKernelGGL(step, grid, block, 0, h->stream, a.u, a.ut, f[0], f[1], f[2], f[3], f[4], f[5], a.vx, a.vy, a.vz, a.nx, a.ny, a.nz, a.eu, a.ew, a.evx,
                           a.evy, a.evz, a._dx, a._dy, a._dz, a.dt);
    }
    return JRX_OK;
}

// The checks of both entry points.  v, vdim: the ND velocities; f: the 2 ND flux arrays -- the fused 3D form keeps every flux in registers and needs only fL
// (its u1), so there fR .. fU may be NULL; the 2D entry point asks for all four in either form.  The velocities are only read and may share memory among
// themselves; no other two arrays may.
jrx_status weno_checks(jrx_handle *h, int ND, const double *u, const int64_t *udim, const double *const *v, const int64_t *const *vdim, const double *ut,
                       double *const *f, const int64_t *wdim, int32_t method)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "WENO_advection!";
    static const char *const vn[3] = {"vx", "vy", "vz"}, *const fname[6] = {"fL", "fR", "fB", "fT", "fD", "fU"};
    bool null = !u || !udim || !ut || !f[0] || !wdim, fluxes = true;
    for (int c = 0; c < ND; c++) null = null || !v[c] || !vdim[c];
    for (int q = 1; q < 2 * ND; q++) fluxes = fluxes && f[q];
    if (null || (ND == 2 && !fluxes)) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (!h->weno_fused && !fluxes) return jrx_fail(h, JRX_ERR_ARG, "%s: the per-kernel form (weno_fused = 0) needs all of fL, fR, fB, fT, fD, fU", fn);
    if (method != 1 && method != 2) return jrx_fail(h, JRX_ERR_ARG, "%s: method must be 1 (JS) or 2 (Z), got %d", fn, (int)method);
    if (!op_extents_ok(udim, ND)) return jrx_fail(h, JRX_ERR_ARG, "%s: size(u) = (%s)", fn, op_list(udim, ND, ", ").s);
    for (int a = 0; a <= ND; a++) {
        const int64_t *dim = a < ND ? vdim[a] : wdim;
        const char *name = a < ND ? vn[a] : ND == 2 ? "weno.ut / fL / fR / fB / fT" : "weno.ut / fL / fR / fB / fT / fD / fU";
        for (int d = 0; d < ND; d++)
            if (dim[d] < udim[d])
                return jrx_fail(h, JRX_ERR_ARG, "%s: %s is smaller than u along dimension %d (%lld < %lld)", fn, name, d + 1, (long long)dim[d], (long long)udim[d]);
    }
    // u, ut and the flux arrays that are there are written; ut stands for the flux arrays in the 2^31 test (they share its extents)
    OpArr out[8] = {{u, 0, "u"}, {ut, 0, "ut"}}, in[3];
    const int64_t *odim[2] = {udim, wdim};
    int nout = 2;
    for (int q = 0; q < 2 * ND; q++)
        if (f[q]) out[nout++] = OpArr{f[q], 0, fname[q]};
    for (int c = 0; c < ND; c++) in[c] = OpArr{v[c], 0, vn[c]};
    for (int a = 0; a < ND + 2; a++) {                          // u, the velocities, ut
        const int64_t *dim = a == 0 ? udim : a <= ND ? vdim[a - 1] : wdim;
        if (op_2g(op_count(dim, ND, 0)))
            return jrx_fail(h, JRX_ERR_UNSUPPORTED, "%s: %s has 2^31 or more entries (32-bit offsets)", fn, a == 0 ? "u" : a <= ND ? vn[a - 1] : "ut");
    }
    for (int m = 0; m < nout; m++) out[m].bytes = op_bytes(odim[m > 0], ND, 0, 0, 0);
    for (int c = 0; c < ND; c++) in[c].bytes = op_bytes(vdim[c], ND, 0, 0, 0);
    if (const OpClash c = op_disjoint(out, nout, in, ND)) {
        if (c.two) return jrx_fail(h, JRX_ERR_ARG, "%s: %s and %s overlap", fn, out[c.a].name, out[c.b].name);
        return c.a == 0 ? jrx_fail(h, JRX_ERR_ARG, "%s: u and %s overlap", fn, in[c.b].name)          // the names in argument order
                        : jrx_fail(h, JRX_ERR_ARG, "%s: %s and %s overlap", fn, in[c.b].name, out[c.a].name);
    }
    return jrx_check_device(h);
}

}  // namespace

extern "C" {

jrx_status jrx_weno5_advection2d(jrx_handle *h, double *u, const int64_t udim[2], const double *vx, const int64_t vxdim[2], const double *vy,
                                 const int64_t vydim[2], double *ut, double *fL, double *fR, double *fB, double *fT, const int64_t wdim[2], double dx, double dy,
                                 double dt, int32_t method)
{
    const double *const v[2] = {vx, vy};
    const int64_t *const vdim[2] = {vxdim, vydim};
    double *const f[4] = {fL, fR, fB, fT};
    JRX_TRY(weno_checks(h, 2, u, udim, v, vdim, ut, f, wdim, method));
    const int nx = (int)udim[0], ny = (int)udim[1], lu = (int)udim[0], lw = (int)wdim[0], lvx = (int)vxdim[0], lvy = (int)vydim[0];
    const double _dx = 1.0 / dx, _dy = 1.0 / dy;                // _di = inv.(di)
    h->stat_weno_calls++;
    if (h->weno_fused) {
        h->stat_weno_fused++;
        if (method == 1) JRX_TRY(launch_fused<1>(h, u, ut, fL, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt));
        else JRX_TRY(launch_fused<2>(h, u, ut, fL, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt));
    } else {
        if (method == 1) JRX_TRY(launch_split<1>(h, u, ut, fL, fR, fB, fT, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt));
        else JRX_TRY(launch_split<2>(h, u, ut, fL, fR, fB, fT, vx, vy, nx, ny, lu, lw, lvx, lvy, _dx, _dy, dt));
    }
    return op_finish(h);
}

jrx_status jrx_weno5_advection3d(jrx_handle *h, double *u, const int64_t udim[3], const double *vx, const int64_t vxdim[3], const double *vy,
                                 const int64_t vydim[3], const double *vz, const int64_t vzdim[3], double *ut, double *fL, double *fR, double *fB, double *fT,
                                 double *fD, double *fU, const int64_t wdim[3], double dx, double dy, double dz, double dt, int32_t method)
{
    const double *const v[3] = {vx, vy, vz};
    const int64_t *const vdim[3] = {vxdim, vydim, vzdim};
    double *const f[6] = {fL, fR, fB, fT, fD, fU};
    JRX_TRY(weno_checks(h, 3, u, udim, v, vdim, ut, f, wdim, method));
    auto ext = [](const int64_t *d) { return WenoExt{(int)d[0], (int)(d[0] * d[1])}; };
    Weno3Args a;
    a.u = u; a.ut = ut; a.f[0] = fL; a.f[1] = fR; a.f[2] = fB; a.f[3] = fT; a.f[4] = fD; a.f[5] = fU;
    a.vx = vx; a.vy = vy; a.vz = vz;
    a.nx = (int)udim[0]; a.ny = (int)udim[1]; a.nz = (int)udim[2];
    a.eu = ext(udim); a.ew = ext(wdim); a.evx = ext(vxdim); a.evy = ext(vydim); a.evz = ext(vzdim);
    a._dx = 1.0 / dx; a._dy = 1.0 / dy; a._dz = 1.0 / dz; a.dt = dt;                // _di = inv.(di)
    h->stat_weno3d_calls++;
    if (h->weno_fused) {
        h->stat_weno3d_fused++;
        JRX_TRY(method == 1 ? launch_fused3d<1>(h, a) : launch_fused3d<2>(h, a));
    } else {
        JRX_TRY(method == 1 ? launch_split3d<1>(h, a) : launch_split3d<2>(h, a));
    }
    return op_finish(h);
}

}  // extern "C"
