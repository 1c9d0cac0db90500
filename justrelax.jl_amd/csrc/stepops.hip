// stepops.hip -- the per-step operators a time loop calls around the solves: pureshear_bc!, free_surface_bcs!, subgrid_characteristic_time!,
// compute_melt_fraction!, for gfx950.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/boundaryconditions/pure_shear.jl:1-33, src/boundaryconditions/free_surface.jl:1-99,
// src/particles/subgrid_diffusion.jl:36-50, src/rheology/Melting.jl:10-35; fn_ratio src/phases/phases.jl:6-30.  Departures and kept quirks: include/jrx.h.
// Every operator is one launch of one thread per output value, x fastest across the lanes of a wave.  pureshear_bc! and free_surface_bcs! touch faces and
// a few planes (launch-bound); the other two stream the cells once (HBM-bound: the ratios, T[, P] in, one value out).
// The library builds with -ffp-contract=off: no fma appears here, so every expression keeps the reference's grouping and roundings.
#include "op_args.hpp"
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

unsigned blocks(i64 n) { return (unsigned)((n + 255) / 256); }

jrx_status phase_g(jrx_handle *h, const char *who, const jrx_rheology *rh, PhaseG *g)
{
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phases (1..%d)", who, (int)rh->nphase, JRX_MAXPHASE);
    g->nphase = rh->nphase;
    for (int q = 0; q < JRX_MAXPHASE; q++) g->G[q] = q < rh->nphase ? rh->G[q] : 0.0;
    return JRX_OK;
}

// pureshear_bc!: V the ND velocity components, x the ND vertex coordinate vectors
jrx_status so_pureshear(jrx_handle *h, int ND, double *const *V, const double *const *x, double eps_bg, const int64_t n[3])
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "pureshear_bc!";
    bool null = false;
    for (int c = 0; c < ND; c++) null = null || !V[c] || !x[c];
    if (null) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (!op_extents_ok(n, ND)) return jrx_fail(h, JRX_ERR_ARG, "%s: ni = (%s)", fn, op_list(n, ND, ", ").s);
    if (op_2g(op_count(n, ND, 2))) return jrx_fail(h, JRX_ERR_ARG, "%s: a velocity array of 2^31 or more entries", fn);
    OpArr out[3], in[3];
    for (int c = 0; c < ND; c++) out[c] = OpArr{V[c], op_vel_bytes(n, ND, c), nullptr}, in[c] = OpArr{x[c], 8 * (n[c] + 1), nullptr};
    if (const OpClash c = op_disjoint(out, ND, in, ND))
        return !c.two ? jrx_fail(h, JRX_ERR_ARG, "%s: a velocity array overlaps a coordinate vector", fn)
                      : jrx_fail(h, JRX_ERR_ARG, ND == 2 ? "%s: Vx and Vy overlap" : "%s: two velocity arrays overlap", fn);
    JRX_TRY(jrx_check_device(h));
    const int nx = (int)n[0], ny = (int)n[1], nz = (int)n[2];
    if (ND == 2) hipLaunchKernelGGL(k_pureshear2d, dim3(blocks(op_bytes(n, 2, 1, 1) / 8)), dim3(256), 0, h->stream, V[0], V[1], x[0], x[1], eps_bg, nx, ny);
    else hipLaunchKernelGGL(k_pureshear3d, dim3(blocks(op_bytes(n, 3, 1, 1, 1) / 8)), dim3(256), 0, h->stream, V[0], V[1], V[2], x[0], x[1], x[2], eps_bg, nx, ny, nz);
    h->stat_stepops_launches++;
    return op_finish(h);
}

// free_surface_bcs!: Vtop the vertical velocity component (written), Vside the ND - 1 others; cen = P, P0, τ_o.yy, η at the cell centres; d the ND spacings, of
// which the 2D kernel reads dx_i / dy_j instead where that array is given
jrx_status so_free_surface(jrx_handle *h, int ND, double *Vtop, const double *const *Vside, const double *const *cen, const double *phase_c, const jrx_rheology *rh,
                           double dt, const double *d, const double *dx_i, const double *dy_j, const int64_t n[3], int32_t free_surface)
{
    if (!h) return JRX_ERR_ARG;
    if (!free_surface) return JRX_OK;
    const char *fn = "free_surface_bcs!";
    const int top = "xyz"[ND - 1];                    // the component written: Vy in 2D, Vz in 3D
    bool null = !Vtop || !phase_c || !rh;
    for (int c = 0; c < ND - 1; c++) null = null || !Vside[c];
    for (int q = 0; q < 4; q++) null = null || !cen[q];
    if (null) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (!op_extents_ok(n, ND)) return jrx_fail(h, JRX_ERR_ARG, "%s: ni = (%s)", fn, op_list(n, ND, ", ").s);
    PhaseG g;
    JRX_TRY(phase_g(h, fn, rh, &g));
    if (op_2g(op_count(n, ND, 2)) || op_2g((double)g.nphase * op_count(n, ND, 0))) return jrx_fail(h, JRX_ERR_ARG, "%s: an array of 2^31 or more entries", fn);
    if (!op_pos_finite(dt)) return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g", fn, dt);
    const double *const per_cell[3] = {dx_i, dy_j, nullptr};
    bool spacings = true;
    for (int a = 0; a < ND; a++) spacings = spacings && (per_cell[a] || op_pos_finite(d[a]));
    if (!spacings) return jrx_fail(h, JRX_ERR_ARG, "%s: spacings (%s)", fn, op_list(d, ND, ", ").s);
    const i64 nc = op_bytes(n, ND, 0, 0, 0);              // bytes of a centre array
    const OpArr out[1] = {{Vtop, op_vel_bytes(n, ND, ND - 1), nullptr}};
    OpArr in[7];
    for (int q = 0; q < 4; q++) in[q] = OpArr{cen[q], nc, nullptr};
    for (int c = 0; c < ND - 1; c++) in[4 + c] = OpArr{Vside[c], op_vel_bytes(n, ND, c), nullptr};
    in[3 + ND] = OpArr{phase_c, g.nphase * nc, nullptr};
    if (const OpClash c = op_disjoint(out, 1, in, 4 + ND))
        return jrx_fail(h, JRX_ERR_ARG, "%s: V%c overlaps %s", fn, top, c.b == 3 + ND ? "the phase ratios" : "an input array");
    JRX_TRY(jrx_check_device(h));
    const int nx = (int)n[0], ny = (int)n[1], nz = (int)n[2];
    if (ND == 2)
        hipLaunchKernelGGL(k_free_surface2d, dim3(blocks(nx)), dim3(256), 0, h->stream, Vside[0], Vtop, cen[0], cen[1], cen[2], cen[3], phase_c, g, dt, d[0], d[1],
                           dx_i, dy_j, nx, ny);
    else
        hipLaunchKernelGGL(k_free_surface3d, dim3(blocks((i64)nx * ny)), dim3(256), 0, h->stream, Vside[0], Vside[1], Vtop, cen[0], cen[1], cen[2], cen[3], phase_c, g,
                           dt, d[0], d[1], d[2], nx, ny, nz);
    h->stat_stepops_launches++;
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_pureshear_bc2d(jrx_handle *h, double *Vx, double *Vy, const double *xv, const double *yv, double eps_bg, int64_t nx, int64_t ny)
{
    double *const V[2] = {Vx, Vy};
    const double *const x[2] = {xv, yv};
    const int64_t n[3] = {nx, ny, 1};
    return so_pureshear(h, 2, V, x, eps_bg, n);
}

jrx_status jrx_pureshear_bc3d(jrx_handle *h, double *Vx, double *Vy, double *Vz, const double *xv, const double *yv, const double *zv, double eps_bg,
                              int64_t nx, int64_t ny, int64_t nz)
{
    double *const V[3] = {Vx, Vy, Vz};
    const double *const x[3] = {xv, yv, zv};
    const int64_t n[3] = {nx, ny, nz};
    return so_pureshear(h, 3, V, x, eps_bg, n);
}

jrx_status jrx_free_surface_bcs2d(jrx_handle *h, const double *Vx, double *Vy, const double *P, const double *P0, const double *tau_o_yy, const double *eta,
                                  const double *phase_c, const jrx_rheology *rh, double dt, double dx, double dy, const double *dx_i, const double *dy_j,
                                  int64_t nx, int64_t ny, int32_t free_surface)
{
    const double *const Vside[1] = {Vx};
    const double *const cen[4] = {P, P0, tau_o_yy, eta};
    const int64_t n[3] = {nx, ny, 1};
    const double d[2] = {dx, dy};
    return so_free_surface(h, 2, Vy, Vside, cen, phase_c, rh, dt, d, dx_i, dy_j, n, free_surface);
}

jrx_status jrx_free_surface_bcs3d(jrx_handle *h, const double *Vx, const double *Vy, double *Vz, const double *P, const double *P0, const double *tau_o_yy,
                                  const double *eta, const double *phase_c, const jrx_rheology *rh, double dt, double dx, double dy, double dz, int64_t nx,
                                  int64_t ny, int64_t nz, int32_t free_surface)
{
    const double *const Vside[2] = {Vx, Vy};
    const double *const cen[4] = {P, P0, tau_o_yy, eta};
    const int64_t n[3] = {nx, ny, nz};
    const double d[3] = {dx, dy, dz};
    return so_free_surface(h, 3, Vz, Vside, cen, phase_c, rh, dt, d, nullptr, nullptr, n, free_surface);
}

jrx_status jrx_subgrid_characteristic_time(jrx_handle *h, double *dt0, const double *phase_c, const jrx_thermal_phases *ph, const double *T, const double *P,
                                           const int64_t n[3], int32_t ndim, const double di[3])
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "subgrid_characteristic_time!";
    if (!dt0 || !phase_c || !ph || !T || !P || !n || !di) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (ndim != 2 && ndim != 3) return jrx_fail(h, JRX_ERR_ARG, "%s: ndim = %d", fn, (int)ndim);
    if (ph->nphase < 1 || ph->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phases (1..%d)", fn, (int)ph->nphase, JRX_MAXPHASE);
    const int64_t m[3] = {n[0], n[1], ndim == 3 ? n[2] : 1};
    if (!op_extents_ok(m, 3)) return jrx_fail(h, JRX_ERR_ARG, "%s: size(stokes.P) = (%s)", fn, op_list(m, 3, ", ").s);
    if (op_2g(op_count(m, ndim, 2)) || op_2g((double)ph->nphase * op_count(m, 3, 0))) return jrx_fail(h, JRX_ERR_ARG, "%s: an array of 2^31 or more entries", fn);
    double sum_dxi = 0.0;          // mapreduce(x -> inv(x)^2, +, di): left to right
    for (int d = 0; d < ndim; d++) {
        if (!op_pos_finite(di[d])) return jrx_fail(h, JRX_ERR_ARG, "%s: di[%d] = %g", fn, d + 1, di[d]);
        const double inv = 1.0 / di[d];
        sum_dxi = d == 0 ? inv * inv : sum_dxi + inv * inv;
    }
    const i64 bytes = op_bytes(m, 3, 0, 0, 0);
    const OpArr out[1] = {{dt0, bytes, nullptr}}, in[3] = {{T, op_bytes(m, ndim, 2, 2, 2), nullptr}, {P, bytes, nullptr}, {phase_c, ph->nphase * bytes, nullptr}};
    if (op_disjoint(out, 1, in, 3)) return jrx_fail(h, JRX_ERR_ARG, "%s: dt₀ overlaps an input array", fn);
    JRX_TRY(jrx_check_device(h));
    const int sk = ndim == 3 ? 1 : 0;
    dispatch_const<0, 1, 2, 3, 4>(ph->nphase <= 4 ? ph->nphase : 0, [&](auto NP) {
        hipLaunchKernelGGL(k_subgrid_time<NP()>, dim3(blocks(bytes / 8)), dim3(256), 0, h->stream, dt0, phase_c, *ph, T, P, sum_dxi, (int)m[0], (int)m[1], (int)m[2], sk);
    });
    h->stat_stepops_launches++;
    return op_finish(h);
}

jrx_status jrx_compute_melt_fraction(jrx_handle *h, double *phi, const double *phase_c, const jrx_melting *m, const double *T, double T_scalar, const double *P,
                                     double P_scalar, const int64_t n[3], int32_t ndim)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "compute_melt_fraction!";
    if (!phi || !m || !n) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (ndim != 2 && ndim != 3) return jrx_fail(h, JRX_ERR_ARG, "%s: ndim = %d", fn, (int)ndim);
    if (m->nphase < 1 || m->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phases (1..%d)", fn, (int)m->nphase, JRX_MAXPHASE);
    for (int q = 0; q < m->nphase; q++)
        if (m->kind[q] != 0 && m->kind[q] != 1)
            return jrx_fail(h, JRX_ERR_ARG, "%s: melting kind %d of phase %d is not built (0 = none, 1 = MeltingParam_Caricchi: the one law the reference's tests pin)",
                            fn, (int)m->kind[q], q + 1);
    const int64_t e[3] = {n[0], n[1], ndim == 3 ? n[2] : 1};
    if (!op_extents_ok(e, 3)) return jrx_fail(h, JRX_ERR_ARG, "%s: size(ϕ) = (%s)", fn, op_list(e, 3, ", ").s);
    if (op_2g((phase_c ? (double)m->nphase : 1.0) * op_count(e, 3, 0))) return jrx_fail(h, JRX_ERR_ARG, "%s: an array of 2^31 or more entries", fn);
    (void)P_scalar;                // neither law reads the pressure
    const i64 bytes = op_bytes(e, 3, 0, 0, 0), nc = bytes / 8;
    const OpArr out[1] = {{phi, bytes, nullptr}};
    OpArr in[3];                   // T, P and the phase ratios: those that are there
    int nin = 0;
    if (T) in[nin++] = OpArr{T, bytes, nullptr};
    if (P) in[nin++] = OpArr{P, bytes, nullptr};
    if (phase_c) in[nin++] = OpArr{phase_c, m->nphase * bytes, nullptr};
    if (op_disjoint(out, 1, in, nin)) return jrx_fail(h, JRX_ERR_ARG, "%s: ϕ overlaps an input array", fn);
    JRX_TRY(jrx_check_device(h));
    if (!phase_c)
        hipLaunchKernelGGL((k_melt_fraction<0, false>), dim3(blocks(nc)), dim3(256), 0, h->stream, phi, phase_c, *m, T, T_scalar, nc);
    else
        dispatch_const<0, 1, 2, 3, 4>(m->nphase <= 4 ? m->nphase : 0, [&](auto NP) {
            hipLaunchKernelGGL((k_melt_fraction<NP(), true>), dim3(blocks(nc)), dim3(256), 0, h->stream, phi, phase_c, *m, T, T_scalar, nc);
        });
    h->stat_stepops_launches++;
    return op_finish(h);
}

}  // extern "C"
