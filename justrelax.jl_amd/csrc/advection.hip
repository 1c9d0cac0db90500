// advection.hip -- WENO-5 advection of a 2D vertex field (WENO_advection!), for gfx950.
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
// Addressing: 32-bit element offsets (every array below 2^31 entries, checked).
#include "jrx_internal.hpp"

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

}  // namespace

extern "C" {

jrx_status jrx_weno5_advection2d(jrx_handle *h, double *u, const int64_t udim[2], const double *vx, const int64_t vxdim[2], const double *vy,
                                 const int64_t vydim[2], double *ut, double *fL, double *fR, double *fB, double *fT, const int64_t wdim[2], double dx, double dy,
                                 double dt, int32_t method)
{
    if (!h) return JRX_ERR_ARG;
    if (!u || !udim || !vx || !vxdim || !vy || !vydim || !ut || !fL || !fR || !fB || !fT || !wdim)
        return jrx_fail(h, JRX_ERR_ARG, "WENO_advection!: NULL argument");
    if (method != 1 && method != 2) return jrx_fail(h, JRX_ERR_ARG, "WENO_advection!: method must be 1 (JS) or 2 (Z), got %d", (int)method);
    if (udim[0] < 1 || udim[1] < 1) return jrx_fail(h, JRX_ERR_ARG, "WENO_advection!: size(u) = (%lld, %lld)", (long long)udim[0], (long long)udim[1]);
    const int64_t *dims[4] = {udim, vxdim, vydim, wdim};
    const char *names[4] = {"u", "vx", "vy", "weno.ut / fL / fR / fB / fT"};
    for (int a = 1; a < 4; a++)
        for (int d = 0; d < 2; d++)
            if (dims[a][d] < udim[d])
                return jrx_fail(h, JRX_ERR_ARG, "WENO_advection!: %s is smaller than u along dimension %d (%lld < %lld)", names[a], d + 1, (long long)dims[a][d],
                                (long long)udim[d]);
    // no two arrays may overlap, except the two read-only velocities
    const void *p[8] = {u, vx, vy, ut, fL, fR, fB, fT};
    const int64_t *pd[8] = {udim, vxdim, vydim, wdim, wdim, wdim, wdim, wdim};
    const char *pn[8] = {"u", "vx", "vy", "ut", "fL", "fR", "fB", "fT"};
    for (int a = 0; a < 8; a++) {
        if ((double)pd[a][0] * (double)pd[a][1] >= 2147483648.0)
            return jrx_fail(h, JRX_ERR_UNSUPPORTED, "WENO_advection!: %s has 2^31 or more entries (32-bit offsets)", pn[a]);
        for (int b = a + 1; b < 8; b++) {
            if (a == 1 && b == 2) continue;
            const char *pa = (const char *)p[a], *pb = (const char *)p[b];
            if (pa < pb + 8 * pd[b][0] * pd[b][1] && pb < pa + 8 * pd[a][0] * pd[a][1])
                return jrx_fail(h, JRX_ERR_ARG, "WENO_advection!: %s and %s overlap", pn[a], pn[b]);
        }
    }
    JRX_TRY(jrx_check_device(h));
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
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

}  // extern "C"
