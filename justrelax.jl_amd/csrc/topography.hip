// topography.hip -- a moving free surface in 2D on grids: rock fractions from a height field (compute_rock_fraction!(ϕ, topo, grid)), its semi-Lagrangian
// advection (advect_topography!(topo, V, grid, dt)) and the phase correction (update_phases_given_topography!(phases, topo, grid, air_phase)), for gfx950.
//
// Reference: none to restate.  The reference's free-surface miniapps (miniapps/DYREL2D/volcano/Caldera2D.jl:175-195,439-449, the Subduction2D_VS* set) call
// JustPIC's marker chain -- fill_chain_from_vertices!, semilagrangian_advection_markerchain!, compute_rock_fraction!(ϕ, chain, xvi, di) -- which is not in the
// reference tree, and update_phases_given_markerchain! (src/phases/topography_correction.jl:64-90) works on particles.  include/jrx.h states the definitions
// built here; tests/_topography.py is the same text in NumPy.
//
// The surface is the polyline through (x_v[i], h[i]), i = 0 .. nx.  All arithmetic is fp64 in cell units, s = (h - y0) _dy; no fma (the library builds with
// -ffp-contract=off): every product and sum is rounded once in the order written, so the device and the NumPy text leave the same bits.
//
// Shapes.  k_rock_fraction2d: ONE launch, a thread per node of the ni .+ 1 box (64 x 4) writes every member of ϕ that node owns (centre, Vx, Vy, vertex); its
// only loads are h[i - 1], h[i], h[i + 1], so the stores are the whole traffic.  k_advect_topography2d: a thread per vertex abscissa.
// k_phases_topography2d<N>: a thread per column marches j = 0 .. ny - 1 and carries the rock proportions of the last cell that had rock; the lanes of a wave
// read and write consecutive x.  Addressing: 32-bit element offsets (every array below 2^31 entries, checked).
#include "jrx_internal.hpp"

namespace {

constexpr int kTpTX = 64, kTpTY = 4;                  // tile of nodes of k_rock_fraction2d
constexpr int kTpCols = 64;                           // columns per block of the 1D kernels

// clamp by comparisons: a NaN becomes lo (so that an index derived from it stays inside its array)
__device__ __forceinline__ double tp_clamp(double x, double lo, double hi) { return x >= lo ? (x <= hi ? x : hi) : lo; }

// Φ(g): the area below a unit-slope ramp clipped to [0, H]
__device__ __forceinline__ double tp_phi(double g, double H) { return g <= 0.0 ? 0.0 : (g < H ? (0.5 * g) * g : H * g - (0.5 * H) * H); }

// area below one linear piece (end heights ga, gb above the volume's bottom) inside a volume of width w and height H, cell units
__device__ __forceinline__ double tp_piece(double ga, double gb, double w, double H)
{
    if (ga == gb) return w * tp_clamp(ga, 0.0, H);
    return (w * (tp_phi(gb, H) - tp_phi(ga, H))) / (gb - ga);
}

__device__ __forceinline__ double tp_height(const double *__restrict__ h, int i, double y0, double idy) { return (h[i] - y0) * idy; }

// center[i, j]: the fraction of cell (i, j) below the segment s0 .. s1
__device__ __forceinline__ double tp_center(double s0, double s1, double j) { return tp_clamp(tp_piece(s0 - j, s1 - j, 1.0, 1.0), 0.0, 1.0); }

struct RfArgs {
    const double *h;
    double *center, *vertex, *Vx, *Vy;
    double y0, idy;
    int nx, ny, nbx;
};

__global__ __launch_bounds__(256) void k_rock_fraction2d(const RfArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int i = ((int)blockIdx.x % a.nbx) * kTpTX + (int)threadIdx.x, j = ((int)blockIdx.x / a.nbx) * kTpTY + (int)threadIdx.y;
    if (i > nx || j > ny) return;
    const bool hasl = i > 0, hasr = i < nx;
    const double s = tp_height(a.h, i, a.y0, a.idy);
    const double sl = hasl ? tp_height(a.h, i - 1, a.y0, a.idy) : s, sr = hasr ? tp_height(a.h, i + 1, a.y0, a.idy) : s;
    const double ml = 0.5 * (sl + s), mr = 0.5 * (s + sr);          // midpoints of the segments i - 1 and i
    const double jd = (double)j;
    const double bj = jd - 0.5, tj = jd + 0.5;
    const double b = bj > 0.0 ? bj : 0.0, t = tj < (double)ny ? tj : (double)ny, H = t - b;      // the volume centred on the vertex row j, clipped to the domain
    const double W = hasl && hasr ? 1.0 : 0.5;
    if (hasr && j < ny) a.center[j * nx + i] = tp_center(s, sr, jd);
    if (hasr) a.Vy[j * nx + i] = tp_clamp(tp_piece(s - b, sr - b, 1.0, H) / H, 0.0, 1.0);
    if (j < ny) {
        const double L = hasl ? tp_piece(ml - jd, s - jd, 0.5, 1.0) : 0.0, R = hasr ? tp_piece(s - jd, mr - jd, 0.5, 1.0) : 0.0;
        a.Vx[j * (nx + 1) + i] = tp_clamp((hasl ? (hasr ? L + R : L) : R) / W, 0.0, 1.0);
    }
    {
        const double L = hasl ? tp_piece(ml - b, s - b, 0.5, H) : 0.0, R = hasr ? tp_piece(s - b, mr - b, 0.5, H) : 0.0;
        a.vertex[j * (nx + 1) + i] = tp_clamp((hasl ? (hasr ? L + R : L) : R) / (W * H), 0.0, 1.0);
    }
}

struct AdvArgs {
    double *h;
    const double *h_old, *Vx, *Vy;      // Vx (nx + 1, ny + 2), Vy (nx + 2, ny + 1)
    double y0, idx, idy, dt;
    int nx, ny;
};

__global__ __launch_bounds__(kTpCols) void k_advect_topography2d(const AdvArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int i = (int)blockIdx.x * kTpCols + (int)threadIdx.x;
    if (i > nx) return;
    const double sig = tp_clamp(tp_height(a.h_old, i, a.y0, a.idy), 0.0, (double)ny);
    int j0 = (int)floor(sig);
    j0 = j0 < ny - 1 ? j0 : ny - 1;
    const double t = sig - (double)j0;
    const double *vxp = a.Vx + j0 * (nx + 1) + i, *vyp = a.Vy + j0 * (nx + 2) + i;
    const double x0 = vxp[0], x1 = vxp[nx + 1], x2 = vxp[2 * (nx + 1)];          // Vx[i, j0 .. j0 + 2]
    const double vx0 = 0.5 * (x0 + x1), vx1 = 0.5 * (x1 + x2);                   // vxv(i, j0), vxv(i, j0 + 1)
    const double vy0 = 0.5 * (vyp[0] + vyp[1]), vy1 = 0.5 * (vyp[nx + 2] + vyp[nx + 3]);
    const double vx = (1.0 - t) * vx0 + t * vx1, vy = (1.0 - t) * vy0 + t * vy1;
    const double xi = tp_clamp((double)i - (vx * a.dt) * a.idx, 0.0, (double)nx);
    int i0 = (int)floor(xi);
    i0 = i0 < nx - 1 ? i0 : nx - 1;
    const double r = xi - (double)i0;
    a.h[i] = ((1.0 - r) * a.h_old[i0] + r * a.h_old[i0 + 1]) + vy * a.dt;
}

struct PhArgs {
    double *c[JRX_MAXPHASE];
    const double *h;
    double y0, idy;
    int nx, ny, air;      // air: 0-based
};

template <int N>
__global__ __launch_bounds__(kTpCols) void k_phases_topography2d(const PhArgs a)
{
    const int nx = a.nx, ny = a.ny, air = a.air;
    const int i = (int)blockIdx.x * kTpCols + (int)threadIdx.x;
    if (i >= nx) return;
    const double s0 = tp_height(a.h, i, a.y0, a.idy), s1 = tp_height(a.h, i + 1, a.y0, a.idy);
    const int first = air == 0 ? 1 : 0;                               // the lowest non-air index (N == 1: none, and no rock field is touched)
    double p[N], c[N];
#pragma unroll
    for (int k = 0; k < N; k++) p[k] = k == first ? 1.0 : 0.0;
    for (int j = 0; j < ny; j++) {
        const int lin = j * nx + i;
        const double f = tp_center(s0, s1, (double)j);
        double R = 0.0, ca = 0.0;
#pragma unroll
        for (int k = 0; k < N; k++) {
            c[k] = a.c[k][lin];
            if (k == air) ca = c[k];
            else R = R + c[k];
        }
        if (R > 0.0) {
#pragma unroll
            for (int k = 0; k < N; k++)
                if (k != air) p[k] = c[k] / R;
        }
        const double airv = 1.0 - f;
        if (ca == airv) continue;
#pragma unroll
        for (int k = 0; k < N; k++) a.c[k][lin] = k == air ? airv : f * p[k];
    }
}

bool tp_overlaps(const void *a, i64 na, const void *b, i64 nb)
{
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + 8 * nb && pb < pa + 8 * na;
}

// extents >= 1 and every array (the largest is the ni .+ 2 box of the velocities) below 2^31 entries
jrx_status tp_extents(jrx_handle *h, const char *fn, int64_t nx, int64_t ny)
{
    if (nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "%s: extents %lld x %lld (each must be >= 1)", fn, (long long)nx, (long long)ny);
    if ((double)(nx + 2) * (double)(ny + 2) >= 2147483648.0) return jrx_fail(h, JRX_ERR_ARG, "%s: the ni .+ 2 box has 2^31 or more entries (32-bit offsets)", fn);
    return JRX_OK;
}

}  // namespace

extern "C" {

jrx_status jrx_compute_rock_fraction2d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *topo_h, int64_t nx, int64_t ny, double y0,
                                       double _dy)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "compute_rock_fraction!";
    double *const out[4] = {center, vertex, Vx, Vy};
    static const char *const names[4] = {"center", "vertex", "Vx", "Vy"};
    for (int m = 0; m < 4; m++)
        if (!out[m]) return jrx_fail(h, JRX_ERR_ARG, "%s: ϕ.%s is NULL", fn, names[m]);
    if (!topo_h) return jrx_fail(h, JRX_ERR_ARG, "%s: topo.h is NULL", fn);
    JRX_TRY(tp_extents(h, fn, nx, ny));
    if (!std::isfinite(y0) || !std::isfinite(_dy)) return jrx_fail(h, JRX_ERR_ARG, "%s: y0 = %g, _dy = %g (both must be finite)", fn, y0, _dy);
    const i64 cnt[4] = {nx * ny, (nx + 1) * (ny + 1), (nx + 1) * ny, nx * (ny + 1)};
    for (int m = 0; m < 4; m++) {
        if (tp_overlaps(out[m], cnt[m], topo_h, nx + 1)) return jrx_fail(h, JRX_ERR_ARG, "%s: output ϕ.%s overlaps topo.h", fn, names[m]);
        for (int q = m + 1; q < 4; q++)
            if (tp_overlaps(out[m], cnt[m], out[q], cnt[q])) return jrx_fail(h, JRX_ERR_ARG, "%s: outputs ϕ.%s and ϕ.%s overlap", fn, names[m], names[q]);
    }
    JRX_TRY(jrx_check_device(h));
    RfArgs a = {topo_h, center, vertex, Vx, Vy, y0, _dy, (int)nx, (int)ny, (int)((nx + 1 + kTpTX - 1) / kTpTX)};
    const int64_t nb = (int64_t)a.nbx * ((ny + 1 + kTpTY - 1) / kTpTY);      // below 2^31: the box is
    h->stat_rock_fraction_calls++;
    hipLaunchKernelGGL(k_rock_fraction2d, dim3((unsigned)nb), dim3(kTpTX, kTpTY), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_advect_topography2d(jrx_handle *h, double *topo_h, double *topo_h_old, const double *Vx, const double *Vy, int64_t nx, int64_t ny, double y0,
                                   double _dx, double _dy, double dt)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "advect_topography!";
    if (!topo_h) return jrx_fail(h, JRX_ERR_ARG, "%s: topo.h is NULL", fn);
    if (!topo_h_old) return jrx_fail(h, JRX_ERR_ARG, "%s: topo.h_old is NULL", fn);
    if (!Vx) return jrx_fail(h, JRX_ERR_ARG, "%s: V.Vx is NULL", fn);
    if (!Vy) return jrx_fail(h, JRX_ERR_ARG, "%s: V.Vy is NULL", fn);
    JRX_TRY(tp_extents(h, fn, nx, ny));
    if (!std::isfinite(dt) || !std::isfinite(_dx) || !std::isfinite(_dy) || !std::isfinite(y0))
        return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g, _dx = %g, _dy = %g, y0 = %g (all must be finite)", fn, dt, _dx, _dy, y0);
    const void *const in[3] = {topo_h_old, Vx, Vy};
    static const char *const names[3] = {"topo.h_old", "V.Vx", "V.Vy"};
    const i64 cnt[3] = {nx + 1, (nx + 1) * (ny + 2), (nx + 2) * (ny + 1)};
    for (int m = 0; m < 3; m++)
        if (tp_overlaps(topo_h, nx + 1, in[m], cnt[m])) return jrx_fail(h, JRX_ERR_ARG, "%s: output topo.h overlaps %s", fn, names[m]);
    for (int m = 1; m < 3; m++)
        if (tp_overlaps(topo_h_old, nx + 1, in[m], cnt[m])) return jrx_fail(h, JRX_ERR_ARG, "%s: output topo.h_old overlaps %s", fn, names[m]);
    JRX_TRY(jrx_check_device(h));
    h->stat_topography_advect_calls++;
    JRX_HIP(h, hipMemcpyAsync(topo_h_old, topo_h, (size_t)(nx + 1) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    AdvArgs a = {topo_h, topo_h_old, Vx, Vy, y0, _dx, _dy, dt, (int)nx, (int)ny};
    hipLaunchKernelGGL(k_advect_topography2d, dim3((unsigned)((nx + 1 + kTpCols - 1) / kTpCols)), dim3(kTpCols), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_update_phases_topography2d(jrx_handle *h, double *const *phases, int32_t nphase, const double *topo_h, int64_t nx, int64_t ny, double y0, double _dy,
                                          int32_t air_phase)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "update_phases_given_topography!";
    if (!phases) return jrx_fail(h, JRX_ERR_ARG, "%s: phases is NULL", fn);
    if (nphase < 1 || nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phase fields (1 .. %d are built)", fn, (int)nphase, JRX_MAXPHASE);
    if (air_phase < 1 || air_phase > nphase) return jrx_fail(h, JRX_ERR_ARG, "%s: air_phase %d outside 1 .. %d", fn, (int)air_phase, (int)nphase);
    for (int k = 0; k < nphase; k++)
        if (!phases[k]) return jrx_fail(h, JRX_ERR_ARG, "%s: phase field %d is NULL", fn, k + 1);
    if (!topo_h) return jrx_fail(h, JRX_ERR_ARG, "%s: topo.h is NULL", fn);
    JRX_TRY(tp_extents(h, fn, nx, ny));
    if (!std::isfinite(y0) || !std::isfinite(_dy)) return jrx_fail(h, JRX_ERR_ARG, "%s: y0 = %g, _dy = %g (both must be finite)", fn, y0, _dy);
    for (int k = 0; k < nphase; k++) {
        if (tp_overlaps(phases[k], nx * ny, topo_h, nx + 1)) return jrx_fail(h, JRX_ERR_ARG, "%s: phase field %d overlaps topo.h", fn, k + 1);
        for (int q = k + 1; q < nphase; q++)
            if (tp_overlaps(phases[k], nx * ny, phases[q], nx * ny)) return jrx_fail(h, JRX_ERR_ARG, "%s: phase fields %d and %d overlap", fn, k + 1, q + 1);
    }
    JRX_TRY(jrx_check_device(h));
    PhArgs a = {};
    for (int k = 0; k < nphase; k++) a.c[k] = phases[k];
    a.h = topo_h, a.y0 = y0, a.idy = _dy, a.nx = (int)nx, a.ny = (int)ny, a.air = (int)air_phase - 1;
    h->stat_topography_phase_calls++;
    dispatch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)nphase, [&](auto NN) {
        hipLaunchKernelGGL((k_phases_topography2d<NN()>), dim3((unsigned)((nx + kTpCols - 1) / kTpCols)), dim3(kTpCols), 0, h->stream, a);
    });
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

}  // extern "C"
