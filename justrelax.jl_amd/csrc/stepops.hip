// stepops.hip -- the per-step operators a time loop calls around the solves: pureshear_bc!, free_surface_bcs!, subgrid_characteristic_time!,
// compute_melt_fraction!, for gfx950.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/boundaryconditions/pure_shear.jl:1-33, src/boundaryconditions/free_surface.jl:1-99,
// src/particles/subgrid_diffusion.jl:36-50, src/rheology/Melting.jl:10-35; fn_ratio src/phases/phases.jl:6-30.  Departures and kept quirks: include/jrx.h.
// Every operator is one launch of one thread per output value, x fastest across the lanes of a wave.  pureshear_bc! and free_surface_bcs! touch faces and
// a few planes (launch-bound); the other two stream the cells once (HBM-bound: the ratios, T[, P] in, one value out).
// The library builds with -ffp-contract=off: no fma appears here, so every expression keeps the reference's grouping and roundings.
#include "jrx_internal.hpp"
#include "jrx_thermal_phases.hpp"

namespace {

// pure_shear.jl:4-5: a thread per node (i, j) of the (nx+1, ny+1) vertex box writes the entry of Vx and of Vy it owns
__global__ __launch_bounds__(256) void k_pureshear2d(double *__restrict__ Vx, double *__restrict__ Vy, const double *__restrict__ xv,
                                                     const double *__restrict__ yv, const double e, const int nx, const int ny)
{
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;          // every array holds fewer than 2^31 entries (checked by the entry point): 32-bit node indices
    const int j = (int)(t / (unsigned)(nx + 1)), i = (int)(t - (unsigned)j * (nx + 1));
    if (j > ny) return;
    if (j < ny) Vx[i + (i64)(nx + 1) * (j + 1)] = e * xv[i];
    if (i < nx) Vy[(i + 1) + (i64)(nx + 2) * j] = -e * yv[j];
}

// pure_shear.jl:16-30 with yv for Vy (include/jrx.h): a thread per node (i, j, k) of the (nx+1, ny+1, nz+1) vertex box
__global__ __launch_bounds__(256) void k_pureshear3d(double *__restrict__ Vx, double *__restrict__ Vy, double *__restrict__ Vz, const double *__restrict__ xv,
                                                     const double *__restrict__ yv, const double *__restrict__ zv, const double e, const int nx, const int ny,
                                                     const int nz)
{
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned plane = (unsigned)(nx + 1) * (ny + 1);
    const int k = (int)(t / plane);
    if (k > nz) return;
    const unsigned r = t - (unsigned)k * plane;
    const int j = (int)(r / (unsigned)(nx + 1)), i = (int)(r - (unsigned)j * (nx + 1));
    if (j < ny && k < nz) Vx[i + (i64)(nx + 1) * ((j + 1) + (i64)(ny + 2) * (k + 1))] = e * xv[i];
    if (i < nx && k < nz) Vy[(i + 1) + (i64)(nx + 2) * (j + (i64)(ny + 1) * (k + 1))] = e * yv[j];
    if (i < nx && j < ny) Vz[(i + 1) + (i64)(nx + 2) * ((j + 1) + (i64)(ny + 2) * k)] = -e * zv[k];
}

// fn_ratio(get_shear_modulus, rheology, ratio): the form without args, phases.jl:6-15
__device__ __forceinline__ double shear_modulus_ratio(const double *__restrict__ G, const double *__restrict__ r, int n)
{
    double x = 0.0;
    for (int q = 0; q < n; q++) x += (r[q] == 0.0) ? 0.0 : G[q] * r[q];
    return x;
}

struct PhaseG { double G[JRX_MAXPHASE]; int nphase; };

// FreeSurface_Vy! 2D, free_surface.jl:38-68: a thread per cell column i; Vx (nx+1, ny+2), Vy (nx+2, ny+1), centre arrays (nx, ny)
__global__ __launch_bounds__(256) void k_free_surface2d(const double *__restrict__ Vx, double *__restrict__ Vy, const double *__restrict__ P,
                                                        const double *__restrict__ P0, const double *__restrict__ toyy, const double *__restrict__ eta,
                                                        const double *__restrict__ phase_c, const PhaseG g, const double dt, const double dx_s,
                                                        const double dy_s, const double *__restrict__ dx_i, const double *__restrict__ dy_j, const int nx,
                                                        const int ny)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nx) return;
    const double dx = dx_i ? dx_i[i] : dx_s, dy = dy_j ? dy_j[ny - 1] : dy_s;
    const i64 c = i + (i64)nx * (ny - 1);
    const double Gdt = shear_modulus_ratio(g.G, phase_c + (i64)g.nphase * c, g.nphase) * dt;
    const double nu = 1.0e-2;
    const i64 top = (i + 1) + (i64)(nx + 2) * ny, below = top - (nx + 2), vx = i + (i64)(nx + 1) * ny;
    Vy[top] = nu * (Vy[below] +
                    (3.0 / 2.0) * (P[c] / (2.0 * eta[c]) + (toyy[c] + P0[c]) / (2.0 * Gdt) + (1.0 / 3.0) * (Vx[vx + 1] - Vx[vx]) * (1.0 / dx)) * dy) +
              (1 - nu) * Vy[top];
}

// FreeSurface_Vy! 3D, free_surface.jl:70-99: a thread per cell column (i, j); Vx (nx+1, ny+2, nz+2), Vy (nx+2, ny+1, nz+2), Vz (nx+2, ny+2, nz+1)
__global__ __launch_bounds__(256) void k_free_surface3d(const double *__restrict__ Vx, const double *__restrict__ Vy, double *__restrict__ Vz,
                                                        const double *__restrict__ P, const double *__restrict__ P0, const double *__restrict__ toyy,
                                                        const double *__restrict__ eta, const double *__restrict__ phase_c, const PhaseG g, const double dt,
                                                        const double dx, const double dy, const double dz, const int nx, const int ny, const int nz)
{
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (int)(t / (unsigned)nx), i = (int)(t - (unsigned)j * nx);
    if (j >= ny) return;
    const i64 c = i + (i64)nx * (j + (i64)ny * (nz - 1));
    const double Gdt = shear_modulus_ratio(g.G, phase_c + (i64)g.nphase * c, g.nphase) * dt;
    const i64 zp = (i64)(nx + 2) * (ny + 2), top = (i + 1) + (i64)(nx + 2) * (j + 1) + zp * nz;
    const i64 vx = i + (i64)(nx + 1) * ((j + 1) + (i64)(ny + 2) * nz), vy = (i + 1) + (i64)(nx + 2) * (j + (i64)(ny + 1) * nz);
    Vz[top] = Vz[top - zp] + 3.0 / 2.0 *
                                 (P[c] / (2.0 * eta[c]) + (toyy[c] + P0[c]) / (2.0 * Gdt) +
                                  (1.0 / 3.0) * ((Vx[vx + 1] - Vx[vx]) * (1.0 / dx) + (Vy[vy + (nx + 2)] - Vy[vy]) * (1.0 / dy))) *
                                 dz;
}

// subgrid_characteristic_time! (subgrid_diffusion.jl:36-50): a thread per cell; T (ni .+ 2) read at I .+ 1, sum_dxi = Σ inv(dx_d)^2 formed on the host as the
// reference's mapreduce does (left to right).  NPH > 0: the phase count as a constant (ratios in one batch of loads), 0: the run-time count
template <int NPH>
__global__ __launch_bounds__(256) void k_subgrid_time(double *__restrict__ dt0, const double *__restrict__ phase_c, const jrx_thermal_phases m,
                                                      const double *__restrict__ T, const double *__restrict__ P, const double sum_dxi, const int nx,
                                                      const int ny, const int nz, const int sk)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (i64)nx * ny * nz) return;
    const unsigned jk = (unsigned)c / (unsigned)nx;                    // fewer than 2^31 cells (checked by the entry point)
    const int i = (int)((unsigned)c - jk * nx), k = (int)(jk / (unsigned)ny), j = (int)(jk - (unsigned)k * ny);
    const double t = T[(i + 1) + (i64)(nx + 2) * ((j + 1) + (i64)(ny + 2) * (k + sk))], p = P[c];
    const double *r = phase_c + (i64)m.nphase * c;
    const double rhoCp = tph_rhoCp<NPH>(m, r, t, p);
    const double K = tph_cond<NPH>(m, r);
    dt0[c] = rhoCp / (2 * K * sum_dxi);
}

// compute_meltfraction of one phase: kind 0 no law, 1 MeltingParam_Caricchi (include/jrx.h)
__device__ __forceinline__ double melt_law(const jrx_melting &m, int q, double T)
{
    if (m.kind[q] == 1) return 1.0 / (1.0 + exp((m.a[q] - (T - m.c[q])) / m.b[q]));
    return 0.0;
}

// compute_melt_fraction_kernel! (Melting.jl:16-20 single material, :29-35 phase ratios): a thread per cell
template <int NPH, bool PH>
__global__ __launch_bounds__(256) void k_melt_fraction(double *__restrict__ phi, const double *__restrict__ phase_c, const jrx_melting m,
                                                       const double *__restrict__ T, const double T_scalar, const i64 n)
{
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double t = T ? T[c] : T_scalar;
    if (!PH) {
        phi[c] = melt_law(m, 0, t);
        return;
    }
    const int np = NPH > 0 ? NPH : m.nphase;
    const TphRatios<NPH> r(phase_c + (i64)np * c);
    double x = 0.0;
    for (int q = 0; q < np; q++) {
        const double rq = r[q];
        if (rq == 1.0) {
            phi[c] = melt_law(m, q, t) * rq;
            return;
        }
        x += (rq == 0.0) ? 0.0 : melt_law(m, q, t) * rq;
    }
    phi[c] = x;
}

bool overlaps(const void *a, i64 na, const void *b, i64 nb)
{
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + 8 * nb && pb < pa + 8 * na;
}

// an extent product as a double: exact far beyond 2^31, never overflows
bool too_many(double entries) { return entries >= 2147483648.0; }
bool pos_finite(double x) { return x > 0.0 && x <= 1.79769313486231570e308; }

unsigned blocks(i64 n) { return (unsigned)((n + 255) / 256); }

jrx_status launched(jrx_handle *h)
{
    h->stat_stepops_launches++;
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status phase_g(jrx_handle *h, const char *who, const jrx_rheology *rh, PhaseG *g)
{
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phases (1..%d)", who, (int)rh->nphase, JRX_MAXPHASE);
    g->nphase = rh->nphase;
    for (int q = 0; q < JRX_MAXPHASE; q++) g->G[q] = q < rh->nphase ? rh->G[q] : 0.0;
    return JRX_OK;
}

}  // namespace

extern "C" {

jrx_status jrx_pureshear_bc2d(jrx_handle *h, double *Vx, double *Vy, const double *xv, const double *yv, double eps_bg, int64_t nx, int64_t ny)
{
    if (!h) return JRX_ERR_ARG;
    if (!Vx || !Vy || !xv || !yv) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: NULL argument");
    if (nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: ni = (%lld, %lld)", (long long)nx, (long long)ny);
    if (too_many(((double)nx + 2) * ((double)ny + 2))) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: a velocity array of 2^31 or more entries");
    const i64 nvx = (nx + 1) * (ny + 2), nvy = (nx + 2) * (ny + 1);
    if (overlaps(Vx, nvx, Vy, nvy)) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: Vx and Vy overlap");
    for (double *o : {Vx, Vy})
        if (overlaps(o, o == Vx ? nvx : nvy, xv, nx + 1) || overlaps(o, o == Vx ? nvx : nvy, yv, ny + 1))
            return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: a velocity array overlaps a coordinate vector");
    JRX_TRY(jrx_check_device(h));
    hipLaunchKernelGGL(k_pureshear2d, dim3(blocks((nx + 1) * (ny + 1))), dim3(256), 0, h->stream, Vx, Vy, xv, yv, eps_bg, (int)nx, (int)ny);
    return launched(h);
}

jrx_status jrx_pureshear_bc3d(jrx_handle *h, double *Vx, double *Vy, double *Vz, const double *xv, const double *yv, const double *zv, double eps_bg,
                              int64_t nx, int64_t ny, int64_t nz)
{
    if (!h) return JRX_ERR_ARG;
    if (!Vx || !Vy || !Vz || !xv || !yv || !zv) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: NULL argument");
    if (nx < 1 || ny < 1 || nz < 1) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: ni = (%lld, %lld, %lld)", (long long)nx, (long long)ny, (long long)nz);
    if (too_many(((double)nx + 2) * ((double)ny + 2) * ((double)nz + 2)))
        return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: a velocity array of 2^31 or more entries");
    double *out[3] = {Vx, Vy, Vz};
    const i64 nout[3] = {(nx + 1) * (ny + 2) * (nz + 2), (nx + 2) * (ny + 1) * (nz + 2), (nx + 2) * (ny + 2) * (nz + 1)};
    const double *in[3] = {xv, yv, zv};
    const i64 nin[3] = {nx + 1, ny + 1, nz + 1};
    for (int a = 0; a < 3; a++) {
        for (int b = a + 1; b < 3; b++)
            if (overlaps(out[a], nout[a], out[b], nout[b])) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: two velocity arrays overlap");
        for (int b = 0; b < 3; b++)
            if (overlaps(out[a], nout[a], in[b], nin[b])) return jrx_fail(h, JRX_ERR_ARG, "pureshear_bc!: a velocity array overlaps a coordinate vector");
    }
    JRX_TRY(jrx_check_device(h));
    hipLaunchKernelGGL(k_pureshear3d, dim3(blocks((nx + 1) * (ny + 1) * (nz + 1))), dim3(256), 0, h->stream, Vx, Vy, Vz, xv, yv, zv, eps_bg, (int)nx, (int)ny,
                       (int)nz);
    return launched(h);
}

jrx_status jrx_free_surface_bcs2d(jrx_handle *h, const double *Vx, double *Vy, const double *P, const double *P0, const double *tau_o_yy, const double *eta,
                                  const double *phase_c, const jrx_rheology *rh, double dt, double dx, double dy, const double *dx_i, const double *dy_j,
                                  int64_t nx, int64_t ny, int32_t free_surface)
{
    if (!h) return JRX_ERR_ARG;
    if (!free_surface) return JRX_OK;
    if (!Vx || !Vy || !P || !P0 || !tau_o_yy || !eta || !phase_c || !rh) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: NULL argument");
    if (nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: ni = (%lld, %lld)", (long long)nx, (long long)ny);
    PhaseG g;
    JRX_TRY(phase_g(h, "free_surface_bcs!", rh, &g));
    if (too_many(((double)nx + 2) * ((double)ny + 2)) || too_many((double)g.nphase * (double)nx * (double)ny))
        return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: an array of 2^31 or more entries");
    if (!pos_finite(dt)) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: dt = %g", dt);
    if ((!dx_i && !pos_finite(dx)) || (!dy_j && !pos_finite(dy))) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: spacings (%g, %g)", dx, dy);
    const i64 nc = nx * ny, nvy = (nx + 2) * (ny + 1);
    const double *in[5] = {P, P0, tau_o_yy, eta, Vx};
    const i64 nin[5] = {nc, nc, nc, nc, (nx + 1) * (ny + 2)};
    for (int q = 0; q < 5; q++)
        if (overlaps(Vy, nvy, in[q], nin[q])) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: Vy overlaps an input array");
    if (overlaps(Vy, nvy, phase_c, g.nphase * nc)) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: Vy overlaps the phase ratios");
    JRX_TRY(jrx_check_device(h));
    hipLaunchKernelGGL(k_free_surface2d, dim3(blocks(nx)), dim3(256), 0, h->stream, Vx, Vy, P, P0, tau_o_yy, eta, phase_c, g, dt, dx, dy, dx_i, dy_j, (int)nx,
                       (int)ny);
    return launched(h);
}

jrx_status jrx_free_surface_bcs3d(jrx_handle *h, const double *Vx, const double *Vy, double *Vz, const double *P, const double *P0, const double *tau_o_yy,
                                  const double *eta, const double *phase_c, const jrx_rheology *rh, double dt, double dx, double dy, double dz, int64_t nx,
                                  int64_t ny, int64_t nz, int32_t free_surface)
{
    if (!h) return JRX_ERR_ARG;
    if (!free_surface) return JRX_OK;
    if (!Vx || !Vy || !Vz || !P || !P0 || !tau_o_yy || !eta || !phase_c || !rh) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: NULL argument");
    if (nx < 1 || ny < 1 || nz < 1) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: ni = (%lld, %lld, %lld)", (long long)nx, (long long)ny, (long long)nz);
    PhaseG g;
    JRX_TRY(phase_g(h, "free_surface_bcs!", rh, &g));
    if (too_many(((double)nx + 2) * ((double)ny + 2) * ((double)nz + 2)) || too_many((double)g.nphase * (double)nx * (double)ny * (double)nz))
        return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: an array of 2^31 or more entries");
    if (!pos_finite(dt)) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: dt = %g", dt);
    if (!pos_finite(dx) || !pos_finite(dy) || !pos_finite(dz)) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: spacings (%g, %g, %g)", dx, dy, dz);
    const i64 nc = nx * ny * nz, nvz = (nx + 2) * (ny + 2) * (nz + 1);
    const double *in[6] = {P, P0, tau_o_yy, eta, Vx, Vy};
    const i64 nin[6] = {nc, nc, nc, nc, (nx + 1) * (ny + 2) * (nz + 2), (nx + 2) * (ny + 1) * (nz + 2)};
    for (int q = 0; q < 6; q++)
        if (overlaps(Vz, nvz, in[q], nin[q])) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: Vz overlaps an input array");
    if (overlaps(Vz, nvz, phase_c, g.nphase * nc)) return jrx_fail(h, JRX_ERR_ARG, "free_surface_bcs!: Vz overlaps the phase ratios");
    JRX_TRY(jrx_check_device(h));
    hipLaunchKernelGGL(k_free_surface3d, dim3(blocks(nx * ny)), dim3(256), 0, h->stream, Vx, Vy, Vz, P, P0, tau_o_yy, eta, phase_c, g, dt, dx, dy, dz, (int)nx,
                       (int)ny, (int)nz);
    return launched(h);
}

jrx_status jrx_subgrid_characteristic_time(jrx_handle *h, double *dt0, const double *phase_c, const jrx_thermal_phases *ph, const double *T, const double *P,
                                           const int64_t n[3], int32_t ndim, const double di[3])
{
    if (!h) return JRX_ERR_ARG;
    if (!dt0 || !phase_c || !ph || !T || !P || !n || !di) return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: NULL argument");
    if (ndim != 2 && ndim != 3) return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: ndim = %d", (int)ndim);
    if (ph->nphase < 1 || ph->nphase > JRX_MAXPHASE)
        return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: %d phases (1..%d)", (int)ph->nphase, JRX_MAXPHASE);
    const int64_t nx = n[0], ny = n[1], nz = ndim == 3 ? n[2] : 1;
    if (nx < 1 || ny < 1 || nz < 1)
        return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: size(stokes.P) = (%lld, %lld, %lld)", (long long)nx, (long long)ny, (long long)nz);
    const double tz = ndim == 3 ? (double)nz + 2 : 1.0;
    if (too_many(((double)nx + 2) * ((double)ny + 2) * tz) || too_many((double)ph->nphase * (double)nx * (double)ny * (double)nz))
        return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: an array of 2^31 or more entries");
    double sum_dxi = 0.0;          // mapreduce(x -> inv(x)^2, +, di): left to right
    for (int d = 0; d < ndim; d++) {
        if (!pos_finite(di[d])) return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: di[%d] = %g", d + 1, di[d]);
        const double inv = 1.0 / di[d];
        sum_dxi = d == 0 ? inv * inv : sum_dxi + inv * inv;
    }
    const i64 nc = nx * ny * nz, nt = (nx + 2) * (ny + 2) * (ndim == 3 ? nz + 2 : 1);
    if (overlaps(dt0, nc, T, nt) || overlaps(dt0, nc, P, nc) || overlaps(dt0, nc, phase_c, ph->nphase * nc))
        return jrx_fail(h, JRX_ERR_ARG, "subgrid_characteristic_time!: dt₀ overlaps an input array");
    JRX_TRY(jrx_check_device(h));
    const int sk = ndim == 3 ? 1 : 0;
    dispatch_const<0, 1, 2, 3, 4>(ph->nphase <= 4 ? ph->nphase : 0, [&](auto NP) {
        hipLaunchKernelGGL(k_subgrid_time<NP()>, dim3(blocks(nc)), dim3(256), 0, h->stream, dt0, phase_c, *ph, T, P, sum_dxi, (int)nx, (int)ny, (int)nz, sk);
    });
    return launched(h);
}

jrx_status jrx_compute_melt_fraction(jrx_handle *h, double *phi, const double *phase_c, const jrx_melting *m, const double *T, double T_scalar, const double *P,
                                     double P_scalar, const int64_t n[3], int32_t ndim)
{
    if (!h) return JRX_ERR_ARG;
    if (!phi || !m || !n) return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: NULL argument");
    if (ndim != 2 && ndim != 3) return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: ndim = %d", (int)ndim);
    if (m->nphase < 1 || m->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: %d phases (1..%d)", (int)m->nphase, JRX_MAXPHASE);
    for (int q = 0; q < m->nphase; q++)
        if (m->kind[q] != 0 && m->kind[q] != 1)
            return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: melting kind %d of phase %d is not built (0 = none, 1 = MeltingParam_Caricchi: the one law "
                                            "the reference's tests pin)", (int)m->kind[q], q + 1);
    const int64_t nx = n[0], ny = n[1], nz = ndim == 3 ? n[2] : 1;
    if (nx < 1 || ny < 1 || nz < 1)
        return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: size(ϕ) = (%lld, %lld, %lld)", (long long)nx, (long long)ny, (long long)nz);
    if (too_many((phase_c ? (double)m->nphase : 1.0) * (double)nx * (double)ny * (double)nz))
        return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: an array of 2^31 or more entries");
    (void)P_scalar;                // neither law reads the pressure
    const i64 nc = nx * ny * nz;
    if ((T && overlaps(phi, nc, T, nc)) || (P && overlaps(phi, nc, P, nc)) || (phase_c && overlaps(phi, nc, phase_c, m->nphase * nc)))
        return jrx_fail(h, JRX_ERR_ARG, "compute_melt_fraction!: ϕ overlaps an input array");
    JRX_TRY(jrx_check_device(h));
    if (!phase_c)
        hipLaunchKernelGGL((k_melt_fraction<0, false>), dim3(blocks(nc)), dim3(256), 0, h->stream, phi, phase_c, *m, T, T_scalar, nc);
    else
        dispatch_const<0, 1, 2, 3, 4>(m->nphase <= 4 ? m->nphase : 0, [&](auto NP) {
            hipLaunchKernelGGL((k_melt_fraction<NP(), true>), dim3(blocks(nc)), dim3(256), 0, h->stream, phi, phase_c, *m, T, T_scalar, nc);
        });
    return launched(h);
}

}  // extern "C"
