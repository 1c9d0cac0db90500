// particles.hip -- 2D marker-in-cell particles in gather form: advection!(particles, RungeKutta2(), V, dt), move_particles!, grid2particle!, particle2grid!
// and update_phase_ratios!(phase_ratios, particles, pPhases); and the elastic stress carried on them: centroid2particle!, particle2centroid!,
// rotate_stress_particles!, rotate_stress!(pτxx, pτyy, pτxy, pω, stokes, particles, dt) and stress2grid!; and the temperature: subgrid_diffusion_centroid! and
// subgrid_diffusion! (operators 10 and 11: Gerya & Yuen's subgrid diffusion, the consumer of subgrid_characteristic_time!); and the refill of thinned cells,
// inject_particles_phase! (operator 12: deterministic, on the empty sites of the seeding lattice; tests/_particles2d_inject.py), for gfx950.
//
// Reference: for the first five none to restate.  The reference's miniapps take them from JustPIC (miniapps/benchmarks/stokes2D/shear_heating/
// Shearheating2D.jl:69-82,221-232 shows the calls), which is not in the reference tree.  include/jrx.h states the definitions built here; tests/_particles2d.py
// is the same text in NumPy.  The stress operators follow the tuple methods of src/stress_rotation/stress_rotation_particles.jl:92-99,224-235,264-276 with
// JustPIC's centroid2particle! / particle2centroid! defined in include/jrx.h (tests/_particles2d_stress.py); the per-point rotation is rotate_point.hpp.
//
// Layout: every per-particle array is (nx, ny, max_xcell) column-major, the slot index slowest (include/jrx.h): a thread owns a cell (or a node) and walks the
// slots, so in every trip of a slot loop the lanes of a wave read consecutive addresses.  An inactive slot holds 0 everywhere.
//
// Every kernel is a gather: a thread writes only what it owns (its cell's slots, its node's members), reads whatever it needs, and every loop is bounded by
// max_xcell or a constant.  Nothing races and nothing depends on launch order; the only atomics are integer adds of per-wave counts into the counter words
// (sums of integers: the order does not matter).  fp64, no fma (-ffp-contract=off): every product and sum is rounded once in the order written.
// An index derived from a coordinate is range-checked on the double before the conversion to int: a NaN or infinite coordinate never reaches a conversion.
// Addressing: 32-bit element offsets (nx ny max_xcell < 2^31, checked).
//
// Launches: 64 x 4 tiles over the box of cells (nx, ny) or of nodes (nx + 1, ny + 1) a kernel covers, in a one-dimensional grid; the kernel hands the x extent
// of its box to pt_index, which derives the block count along x from it as pt_blocks does on the host.  The geometry struct carries no launch parameter.
// Host side: the checks shared with particles3d.hip are in particles_common.hpp (the particle set, the overlap rules, move, phase ratios, the counter read-back);
// here are the conversion of jrx_particles2d (pt_geom), one launcher (pt_launch), one path for the four field operators (pt_field_op) and the entry points.
//
// k_pt_phase_ratios<N>: the phase count is a template argument (1 .. JRX_MAXPHASE) and the phase index of a particle is applied by an unrolled select, so the
// 4 N + 4 accumulators of a node stay in registers (a run-time index into them would put them in scratch).
#include "particles_common.hpp"          // the helpers shared with particles3d.hip
#include "rotate_point.hpp"

namespace {

constexpr int kPtTX = 64, kPtTY = 4;                  // tile of cells / nodes: 64 x 4

struct PtGeom {                                       // jrx_particles2d by value, 32-bit extents
    double *px, *py;
    int *active;
    double x0, y0, dx, dy, idx, idy;
    int nx, ny, mx;                                   // mx = max_xcell
};

// tiles over an (ex, ey) box, row after row of tiles in a one-dimensional grid (no 65535 limit along y); pt_index is its inverse
unsigned pt_blocks(int ex, int ey) { return (unsigned)((i64)((ex + kPtTX - 1) / kPtTX) * ((ey + kPtTY - 1) / kPtTY)); }

// the cell or node (i, j) of a thread in a launch over a box ex wide: a cell kernel passes nx, a node kernel nx + 1
__device__ __forceinline__ void pt_index(int ex, int &i, int &j)
{
    const int nbx = (ex + kPtTX - 1) / kPtTX;
    i = ((int)blockIdx.x % nbx) * kPtTX + (int)threadIdx.x;
    j = ((int)blockIdx.x / nbx) * kPtTY + (int)threadIdx.y;
}

// where (x, y) sits on a node grid of extents (mx, my) and origin (ox, oy): offset of the pair's first node and the local coordinates; false when a scaled
// coordinate is not finite
__device__ __forceinline__ bool pt_locate(int mx, int my, double ox, double oy, double idx, double idy, double x, double y, int &off, double &tx, double &ty)
{
    const double sx = (x - ox) * idx, sy = (y - oy) * idy;
    if (!pt_finite(sx) || !pt_finite(sy)) return false;
    const int i0 = pt_pair(sx, mx), j0 = pt_pair(sy, my);
    tx = sx - (double)i0, ty = sy - (double)j0;
    off = j0 * mx + i0;
    return true;
}

__device__ __forceinline__ double pt_at(const double *__restrict__ A, int mx, int off, double tx, double ty)
{
    const double *p = A + off;
    const double v00 = p[0], v10 = p[1], v01 = p[mx], v11 = p[mx + 1];
    return pt_bilin(tx, ty, v00, v10, v01, v11);
}

// one staggered component A of extents (mx, my), node grid origin (ox, oy), at (x, y); false (and no load) when a scaled coordinate is not finite
__device__ __forceinline__ bool pt_interp(const double *__restrict__ A, int mx, int my, double ox, double oy, double idx, double idy, double x, double y, double &v)
{
    int off;
    double tx, ty;
    if (!pt_locate(mx, my, ox, oy, idx, idy, x, y, off, tx, ty)) return false;
    v = pt_at(A, mx, off, tx, ty);
    return true;
}

// ------------------------------------------------------------------------------------------------ 1. advection, midpoint rule
struct PtAdvArgs {
    PtGeom g;
    const double *Vx, *Vy;
    double oyx, oxy;          // y origin of the Vx nodes (y0 - 0.5 dy), x origin of the Vy nodes (x0 - 0.5 dx)
    double dt, hdt;           // dt, 0.5 dt
};

__global__ __launch_bounds__(256) void k_pt_advect_rk2(const PtAdvArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        const double x = g.px[lin], y = g.py[lin];
        double ux, uy, wx, wy;
        if (!pt_interp(a.Vx, g.nx + 1, g.ny + 2, g.x0, a.oyx, g.idx, g.idy, x, y, ux)) continue;
        if (!pt_interp(a.Vy, g.nx + 2, g.ny + 1, a.oxy, g.y0, g.idx, g.idy, x, y, uy)) continue;
        const double xm = x + a.hdt * ux, ym = y + a.hdt * uy;
        if (!pt_interp(a.Vx, g.nx + 1, g.ny + 2, g.x0, a.oyx, g.idx, g.idy, xm, ym, wx)) continue;
        if (!pt_interp(a.Vy, g.nx + 2, g.ny + 1, a.oxy, g.y0, g.idx, g.idy, xm, ym, wy)) continue;
        g.px[lin] = x + a.dt * wx;
        g.py[lin] = y + a.dt * wy;
    }
}

// ------------------------------------------------------------------------------------------------ 2. move: a destination cell gathers its particles
struct PtMoveArgs {
    PtGeom src;
    double *dpx, *dpy;
    int *dactive;
    const double *as[JRX_MAXPHASE];
    double *ad[JRX_MAXPHASE];
    int nargs;
    unsigned long long *counts;      // n_active_before, n_active_after, n_outside, n_far, n_overflow
};

// owner cell of (x, y): 0 outside the grid, 1 inside (ic, jc set)
__device__ __forceinline__ bool pt_owner(const PtGeom &g, double x, double y, int &ic, int &jc)
{
    const double fx = floor((x - g.x0) * g.idx), fy = floor((y - g.y0) * g.idy);
    if (!(fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny)) return false;
    ic = (int)fx, jc = (int)fy;
    return true;
}

__device__ __forceinline__ void pt_place(const PtMoveArgs &a, int from, int to, double x, double y)
{
    a.dpx[to] = x, a.dpy[to] = y, a.dactive[to] = 1;
#pragma unroll
    for (int k = 0; k < JRX_MAXPHASE; k++)
        if (k < a.nargs) a.ad[k][to] = a.as[k][from];
}

__global__ __launch_bounds__(256) void k_pt_move(const PtMoveArgs a)
{
    const PtGeom &g = a.src;
    int i, j;
    pt_index(g.nx, i, j);
    const bool live = i < g.nx && j < g.ny;
    const int nc = g.nx * g.ny, mx = g.mx;
    int n = 0, n_before = 0, n_outside = 0, n_far = 0, n_overflow = 0;
    if (live) {
        const int base = j * g.nx + i;
        // the cell's own particles first: they always fit
        for (int s = 0, lin = base; s < mx; s++, lin += nc) {
            if (g.active[lin] == 0) continue;
            n_before++;
            const double x = g.px[lin], y = g.py[lin];
            int ic, jc;
            if (!pt_owner(g, x, y, ic, jc)) { n_outside++; continue; }
            const int di = ic - i, dj = jc - j;
            if (di < -1 || di > 1 || dj < -1 || dj > 1) { n_far++; continue; }
            if (di == 0 && dj == 0) {
                pt_place(a, lin, base + n * nc, x, y);
                n++;
            }
        }
        // then the eight neighbours, dj outermost
        for (int dj = -1; dj <= 1; dj++) {
            const int jn = j + dj;
            if (jn < 0 || jn >= g.ny) continue;
            for (int di = -1; di <= 1; di++) {
                const int in = i + di;
                if ((di == 0 && dj == 0) || in < 0 || in >= g.nx) continue;
                for (int s = 0, lin = jn * g.nx + in; s < mx; s++, lin += nc) {
                    if (g.active[lin] == 0) continue;
                    const double x = g.px[lin], y = g.py[lin];
                    int ic, jc;
                    if (!pt_owner(g, x, y, ic, jc) || ic != i || jc != j) continue;
                    if (n < mx) {
                        pt_place(a, lin, base + n * nc, x, y);
                        n++;
                    } else {
                        n_overflow++;
                    }
                }
            }
        }
        for (int s = n, to = base + n * nc; s < mx; s++, to += nc) {
            a.dpx[to] = 0.0, a.dpy[to] = 0.0, a.dactive[to] = 0;
#pragma unroll
            for (int k = 0; k < JRX_MAXPHASE; k++)
                if (k < a.nargs) a.ad[k][to] = 0.0;
        }
    }
    pt_count(a.counts + 0, n_before);
    pt_count(a.counts + 1, n);
    pt_count(a.counts + 2, n_outside);
    pt_count(a.counts + 3, n_far);
    pt_count(a.counts + 4, n_overflow);
}

// ------------------------------------------------------------------------------------------------ 3. grid2particle
struct PtFieldArgs {          // operators 3, 4, 6, 7: a particle field and a grid field; which is written depends on the operator
    PtGeom g;
    double *pF;
    double *F;                // vertices (nx + 1, ny + 1) for operators 3 and 4, centres (nx, ny) for 6 and 7
    double ox, oy;            // origin of the centre nodes (x0 + 0.5 dx, y0 + 0.5 dy)
};

__global__ __launch_bounds__(256) void k_pt_grid2particle(const PtFieldArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    const double *f = a.F + j * (g.nx + 1) + i;
    const double f00 = f[0], f10 = f[1], f01 = f[g.nx + 1], f11 = f[g.nx + 2];
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        double v = 0.0;
        if (g.active[lin] != 0) {
            const double tx = (g.px[lin] - xv) * g.idx, ty = (g.py[lin] - yv) * g.idy;
            v = pt_bilin(tx, ty, f00, f10, f01, f11);
        }
        a.pF[lin] = v;
    }
}

// ------------------------------------------------------------------------------------------------ 4. particle2grid
__global__ __launch_bounds__(256) void k_pt_particle2grid(const PtFieldArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx + 1, i, j);
    if (i > g.nx || j > g.ny) return;
    const int nc = g.nx * g.ny;
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int oi = -1; oi <= 0; oi++) {
#pragma unroll
        for (int oj = -1; oj <= 0; oj++) {
            const int ic = i + oi, jc = j + oj;
            if (ic < 0 || ic >= g.nx || jc < 0 || jc >= g.ny) continue;
            for (int s = 0, lin = jc * g.nx + ic; s < g.mx; s++, lin += nc) {
                if (g.active[lin] == 0) continue;
                const double w = pt_w(g.px[lin], xv, g.idx) * pt_w(g.py[lin], yv, g.idy);
                num += w * a.pF[lin];
                den += w;
            }
        }
    }
    if (!(den == 0.0)) a.F[j * (g.nx + 1) + i] = num / den;
}

// ------------------------------------------------------------------------------------------------ 5. phase ratios
struct PtPrArgs {
    PtGeom g;
    double *center, *vertex, *Vx, *Vy;
    const double *pPhases;
    unsigned long long *n_empty;
};

template <int N>
__device__ __forceinline__ void pt_add(double (&acc)[N], double &W, int k, double w)
{
#pragma unroll
    for (int q = 0; q < N; q++) acc[q] = q == k ? acc[q] + w : acc[q];
    W += w;
}

// ratio_k = w_k / W into N contiguous doubles; 1 (and nothing written) where W == 0
template <int N>
__device__ __forceinline__ int pt_ratio(const double (&acc)[N], double W, double *__restrict__ out)
{
    if (W == 0.0) return 1;
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = acc[q] / W;
    return 0;
}

template <int N>
__global__ __launch_bounds__(256) void k_pt_phase_ratios(const PtPrArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx + 1, i, j);
    const bool live = i <= g.nx && j <= g.ny;
    int empty = 0;
    if (live) {
        const int nc = g.nx * g.ny;
        const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
        const double xc = g.x0 + ((double)i + 0.5) * g.dx, yc = g.y0 + ((double)j + 0.5) * g.dy;
        double ac[N], av[N], ax[N], ay[N];
        double Wc = 0.0, Wv = 0.0, Wx = 0.0, Wy = 0.0;
#pragma unroll
        for (int q = 0; q < N; q++) ac[q] = av[q] = ax[q] = ay[q] = 0.0;
#pragma unroll
        for (int oi = -1; oi <= 0; oi++) {
#pragma unroll
            for (int oj = -1; oj <= 0; oj++) {
                const int ic = i + oi, jc = j + oj;
                if (ic < 0 || ic >= g.nx || jc < 0 || jc >= g.ny) continue;
                for (int s = 0, lin = jc * g.nx + ic; s < g.mx; s++, lin += nc) {
                    if (g.active[lin] == 0) continue;
                    const double p = a.pPhases[lin];
                    if (!(p >= 1.0 && p < (double)(N + 1))) continue;
                    const int k = (int)p - 1;
                    const double x = g.px[lin], y = g.py[lin];
                    const double wxv = pt_w(x, xv, g.idx), wyv = pt_w(y, yv, g.idy);
                    pt_add<N>(av, Wv, k, wxv * wyv);
                    if (oi == 0 || oj == 0) {                       // compile-time after unrolling: the own cell feeds every member, (i-1, j) Vx, (i, j-1) Vy
                        const double wxc = pt_w(x, xc, g.idx), wyc = pt_w(y, yc, g.idy);
                        if (oj == 0) pt_add<N>(ax, Wx, k, wxv * wyc);
                        if (oi == 0) pt_add<N>(ay, Wy, k, wxc * wyv);
                        if (oi == 0 && oj == 0) pt_add<N>(ac, Wc, k, wxc * wyc);
                    }
                }
            }
        }
        const bool hx = i < g.nx, hy = j < g.ny;
        if (hx && hy) empty += pt_ratio<N>(ac, Wc, a.center + (size_t)(j * g.nx + i) * N);
        empty += pt_ratio<N>(av, Wv, a.vertex + (size_t)(j * (g.nx + 1) + i) * N);
        if (hy) empty += pt_ratio<N>(ax, Wx, a.Vx + (size_t)(j * (g.nx + 1) + i) * N);
        if (hx) empty += pt_ratio<N>(ay, Wy, a.Vy + (size_t)(j * g.nx + i) * N);
    }
    pt_count(a.n_empty, empty);
}

// ------------------------------------------------------------------------------------------------ 6. centroid2particle
__global__ __launch_bounds__(256) void k_pt_centroid2particle(const PtFieldArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) {
            a.pF[lin] = 0.0;
            continue;
        }
        double v;
        if (pt_interp(a.F, g.nx, g.ny, a.ox, a.oy, g.idx, g.idy, g.px[lin], g.py[lin], v)) a.pF[lin] = v;
    }
}

// ------------------------------------------------------------------------------------------------ 7. particle2centroid
__global__ __launch_bounds__(256) void k_pt_particle2centroid(const PtFieldArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    const double xc = g.x0 + ((double)i + 0.5) * g.dx, yc = g.y0 + ((double)j + 0.5) * g.dy;
    double num = 0.0, den = 0.0;
    for (int s = 0, lin = j * g.nx + i; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        const double w = pt_w(g.px[lin], xc, g.idx) * pt_w(g.py[lin], yc, g.idy);
        num += w * a.pF[lin];
        den += w;
    }
    if (!(den == 0.0)) a.F[j * g.nx + i] = num / den;
}

// ------------------------------------------------------------------------------------------------ 8. rotation of the particle stress, in place
struct PtRotArgs {
    PtGeom g;
    double *pxx, *pyy, *pxy, *pw;                 // the chain reads pw; the fused kernel writes it
    const double *txx, *tyy, *txy, *wxy;          // fused kernel only: centre fields (nx, ny), vertex fields (nx + 1, ny + 1)
    double ox, oy;                                // origin of the centre nodes
    double dt;
};

template <int METHOD>
__global__ __launch_bounds__(256) void k_pt_rotate(const PtRotArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        double oxx, oyy, oxy;
        rs_rot2<METHOD>(a.pxx[lin], a.pyy[lin], a.pxy[lin], a.dt * a.pw[lin], oxx, oyy, oxy);
        a.pxx[lin] = oxx, a.pyy[lin] = oyy, a.pxy[lin] = oxy;
    }
}

// ------------------------------------------------------------------------------------------------ 9a. rotate_stress!: operators 6, 6, 3, 3, 8 in one launch
// A slot reads active, x, y once.  The centre pair of (x, y) is located once for xx and yy (the same node grid: the same offset and local coordinates as two calls
// of pt_interp); the four vertex values of xy and ω are the bucket cell's, loaded once per thread.  A slot whose scaled coordinate is not finite keeps its xx and
// yy as the chain does -- they are then read -- and still takes xy and ω from the vertices and goes through the rotation.
template <int METHOD>
__global__ __launch_bounds__(256) void k_pt_rotate_stress(const PtRotArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    const double *fs = a.txy + j * (g.nx + 1) + i, *fw = a.wxy + j * (g.nx + 1) + i;
    const double s00 = fs[0], s10 = fs[1], s01 = fs[g.nx + 1], s11 = fs[g.nx + 2];
    const double w00 = fw[0], w10 = fw[1], w01 = fw[g.nx + 1], w11 = fw[g.nx + 2];
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) {
            a.pxx[lin] = 0.0, a.pyy[lin] = 0.0, a.pxy[lin] = 0.0, a.pw[lin] = 0.0;
            continue;
        }
        const double x = g.px[lin], y = g.py[lin];
        int off;
        double cx, cy, xx, yy;
        if (pt_locate(g.nx, g.ny, a.ox, a.oy, g.idx, g.idy, x, y, off, cx, cy)) {
            xx = pt_at(a.txx, g.nx, off, cx, cy);
            yy = pt_at(a.tyy, g.nx, off, cx, cy);
        } else {
            xx = a.pxx[lin], yy = a.pyy[lin];
        }
        const double tx = (x - xv) * g.idx, ty = (y - yv) * g.idy;
        const double xy = pt_bilin(tx, ty, s00, s10, s01, s11);
        const double w = pt_bilin(tx, ty, w00, w10, w01, w11);
        double oxx, oyy, oxy;
        rs_rot2<METHOD>(xx, yy, xy, a.dt * w, oxx, oyy, oxy);
        a.pxx[lin] = oxx, a.pyy[lin] = oyy, a.pxy[lin] = oxy, a.pw[lin] = w;
    }
}

// ------------------------------------------------------------------------------------------------ 9b. stress2grid!: operator 7 three times and operator 4 three times in one launch
struct PtS2GArgs {
    PtGeom g;
    double *cxx, *cyy, *cxy;          // centres (nx, ny): τ_o.xx, yy, xy_c
    double *vxx, *vyy, *vxy;          // vertices (nx + 1, ny + 1): τ_o.xx_v, yy_v, xy
    const double *pxx, *pyy, *pxy;
};

// A thread per node of the (nx + 1, ny + 1) box, the cells of operator 4 in its order; the own cell (i, j) comes last and also feeds the centre the thread owns,
// in slot order as operator 7 walks it.  The three fields of a location share their weights, so one denominator each: eight accumulators.
__global__ __launch_bounds__(256) void k_pt_stress2grid(const PtS2GArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx + 1, i, j);
    if (i > g.nx || j > g.ny) return;
    const int nc = g.nx * g.ny;
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    const double xc = g.x0 + ((double)i + 0.5) * g.dx, yc = g.y0 + ((double)j + 0.5) * g.dy;
    double nvxx = 0.0, nvyy = 0.0, nvxy = 0.0, dv = 0.0;
    double ncxx = 0.0, ncyy = 0.0, ncxy = 0.0, dc = 0.0;
#pragma unroll
    for (int oi = -1; oi <= 0; oi++) {
#pragma unroll
        for (int oj = -1; oj <= 0; oj++) {
            const int ic = i + oi, jc = j + oj;
            if (ic < 0 || ic >= g.nx || jc < 0 || jc >= g.ny) continue;
            for (int s = 0, lin = jc * g.nx + ic; s < g.mx; s++, lin += nc) {
                if (g.active[lin] == 0) continue;
                const double x = g.px[lin], y = g.py[lin];
                const double xx = a.pxx[lin], yy = a.pyy[lin], xy = a.pxy[lin];
                const double w = pt_w(x, xv, g.idx) * pt_w(y, yv, g.idy);
                nvxx += w * xx, nvyy += w * yy, nvxy += w * xy;
                dv += w;
                if (oi == 0 && oj == 0) {          // compile-time after unrolling
                    const double wc = pt_w(x, xc, g.idx) * pt_w(y, yc, g.idy);
                    ncxx += wc * xx, ncyy += wc * yy, ncxy += wc * xy;
                    dc += wc;
                }
            }
        }
    }
    if (!(dv == 0.0)) {
        const int lin = j * (g.nx + 1) + i;
        a.vxx[lin] = nvxx / dv, a.vyy[lin] = nvyy / dv, a.vxy[lin] = nvxy / dv;
    }
    if (i < g.nx && j < g.ny && !(dc == 0.0)) {
        const int lin = j * g.nx + i;
        a.cxx[lin] = ncxx / dc, a.cyy[lin] = ncyy / dc, a.cxy[lin] = ncxy / dc;
    }
}

// ------------------------------------------------------------------------------------------------ 10. / 11. subgrid diffusion of the particle temperature
// VERTEX = false: subgrid_diffusion_centroid! (operators 6 and 7 inside); true: subgrid_diffusion! with loc = :vertex (operators 3 and 4 inside).
struct PtSgArgs {
    PtGeom g;
    double *pT, *pT0, *pdT;       // pT0, pdT: subgrid_arrays.pT0, .pΔT
    const double *pdt0;           // subgrid_arrays.dt₀
    const double *T;              // T_grid: (nx, ny) or (nx + 1, ny + 1)
    const double *dTg;            // ΔT_grid: node (i, j) of the form's node box at dTg[dto + j * dtn + i]
    double *dTs;                  // subgrid_arrays.ΔT_subgrid, the extents of T
    int dtn, dto;
    double ox, oy;                // origin of the centre nodes
    double ndt;                   // (-d) dt, formed once on the host
};

// step 3 of the definition: δ of a slot from the interpolated and the carried temperature
__device__ __forceinline__ double pt_sg_delta(double pTn, double p0, double a, double ndt)
{
    const double m = a > 1e-9 ? a : 1e-9;          // a NaN compares false: the floor
    const double f = 1.0 - exp(ndt / m);
    return (pTn - p0) * f;
}

// the chain's own launches: steps 1, 3, 5 and 7 (steps 2, 4 and 6 are the launches of operators 6 / 3 and 7 / 4)
__global__ __launch_bounds__(256) void k_pt_sg_copy(const PtSgArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) a.pT0[lin] = a.pT[lin];
}

__global__ __launch_bounds__(256) void k_pt_sg_delta(const PtSgArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) {
            a.pdT[lin] = 0.0;
            continue;
        }
        const double p0 = a.pT0[lin];
        const double dl = pt_sg_delta(a.pT[lin], p0, a.pdt0[lin], a.ndt);
        a.pT0[lin] = p0 + dl;
        a.pdT[lin] = dl;
    }
}

// a thread per node of the (ex, ey) box: ΔT_subgrid = ΔT_grid - ΔT_subgrid
__global__ __launch_bounds__(256) void k_pt_sg_remainder(const PtSgArgs a, int ex, int ey)
{
    int i, j;
    pt_index(ex, i, j);
    if (i >= ex || j >= ey) return;
    const int k = j * ex + i;
    a.dTs[k] = a.dTg[a.dto + j * a.dtn + i] - a.dTs[k];
}

__global__ __launch_bounds__(256) void k_pt_sg_add(const PtSgArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) a.pT[lin] = g.active[lin] != 0 ? a.pT0[lin] + a.pdT[lin] : 0.0;
}

// The fused forms.  First launch, a thread per cell, one walk of its bucket: steps 1 - 3 per slot.  Centre form: the same thread accumulates num and den of operator
// 7 in slot order (it reads only this bucket) and writes the cell's remainder, steps 4 and 5; δ goes to memory only where the last launch will need it, in a slot
// whose scaled coordinate is not finite (it finds that out as this launch does, from the same numbers).  The interpolated temperature of step 2 lives in a register:
// pT is written by the last launch alone.  Vertex form: δ of every slot goes to pΔT for the four-cell gather of the second launch.
template <bool VERTEX>
__global__ __launch_bounds__(256) void k_pt_sg_cell(const PtSgArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    double f00 = 0.0, f10 = 0.0, f01 = 0.0, f11 = 0.0;
    if (VERTEX) {
        const double *f = a.T + j * (g.nx + 1) + i;
        f00 = f[0], f10 = f[1], f01 = f[g.nx + 1], f11 = f[g.nx + 2];
    }
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    const double xc = g.x0 + ((double)i + 0.5) * g.dx, yc = g.y0 + ((double)j + 0.5) * g.dy;
    double num = 0.0, den = 0.0;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        const double p0 = a.pT[lin];
        if (g.active[lin] == 0) {
            a.pT0[lin] = p0;
            if (VERTEX) a.pdT[lin] = 0.0;
            continue;
        }
        const double x = g.px[lin], y = g.py[lin];
        double pTn = p0;
        bool ok = true;
        if (VERTEX) pTn = pt_bilin((x - xv) * g.idx, (y - yv) * g.idy, f00, f10, f01, f11);
        else ok = pt_interp(a.T, g.nx, g.ny, a.ox, a.oy, g.idx, g.idy, x, y, pTn);
        const double dl = pt_sg_delta(pTn, p0, a.pdt0[lin], a.ndt);
        a.pT0[lin] = p0 + dl;
        if (VERTEX) {
            a.pdT[lin] = dl;
        } else {
            if (!ok) a.pdT[lin] = dl;
            const double w = pt_w(x, xc, g.idx) * pt_w(y, yc, g.idy);
            num += w * dl;
            den += w;
        }
    }
    if (!VERTEX) {
        const int k = j * g.nx + i;
        a.dTs[k] = a.dTg[a.dto + j * a.dtn + i] - (den == 0.0 ? 0.0 : num / den);
    }
}

// vertex form, second launch: a thread per vertex, the four-cell gather of operator 4 over pΔT and the subtraction of step 5
__global__ __launch_bounds__(256) void k_pt_sg_vertex(const PtSgArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx + 1, i, j);
    if (i > g.nx || j > g.ny) return;
    const int nc = g.nx * g.ny;
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int oi = -1; oi <= 0; oi++) {
#pragma unroll
        for (int oj = -1; oj <= 0; oj++) {
            const int ic = i + oi, jc = j + oj;
            if (ic < 0 || ic >= g.nx || jc < 0 || jc >= g.ny) continue;
            for (int s = 0, lin = jc * g.nx + ic; s < g.mx; s++, lin += nc) {
                if (g.active[lin] == 0) continue;
                const double w = pt_w(g.px[lin], xv, g.idx) * pt_w(g.py[lin], yv, g.idy);
                num += w * a.pdT[lin];
                den += w;
            }
        }
    }
    a.dTs[j * (g.nx + 1) + i] = a.dTg[a.dto + j * a.dtn + i] - (den == 0.0 ? 0.0 : num / den);
}

// last launch, a thread per cell: steps 6 and 7 -- the remainder back to the slots (it reads the neighbours' nodes: hence a launch of its own) and pT = pT0 + pΔT
template <bool VERTEX>
__global__ __launch_bounds__(256) void k_pt_sg_back(const PtSgArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    if (i >= g.nx || j >= g.ny) return;
    const int nc = g.nx * g.ny;
    double f00 = 0.0, f10 = 0.0, f01 = 0.0, f11 = 0.0;
    if (VERTEX) {
        const double *f = a.dTs + j * (g.nx + 1) + i;
        f00 = f[0], f10 = f[1], f01 = f[g.nx + 1], f11 = f[g.nx + 2];
    }
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy;
    int lin = j * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) {
            a.pdT[lin] = 0.0, a.pT[lin] = 0.0;
            continue;
        }
        const double x = g.px[lin], y = g.py[lin];
        double v;
        if (VERTEX) {
            v = pt_bilin((x - xv) * g.idx, (y - yv) * g.idy, f00, f10, f01, f11);
            a.pdT[lin] = v;
        } else if (pt_interp(a.dTs, g.nx, g.ny, a.ox, a.oy, g.idx, g.idy, x, y, v)) {
            a.pdT[lin] = v;
        } else {
            v = a.pdT[lin];          // δ, as the first launch left it
        }
        a.pT[lin] = a.pT0[lin] + v;
    }
}

// ------------------------------------------------------------------------------------------------ 12. injection into deficient cells
struct PtInjArgs {
    PtGeom g;
    int *aout;                            // the mask, out of place
    double *pph;
    double *args[JRX_MAXPHASE];
    const double *fields[JRX_MAXPHASE];
    int loc[JRX_MAXPHASE];
    int nargs, minx, nsx, nsy;
    double hx, hy;                        // dx / nsx, dy / nsy, formed once on the host
    double ox, oy;                        // origin of the centre nodes
    unsigned long long *counts;           // three words: n_active_before | n_active_after << 32, n_deficient | n_injected << 32, n_no_donor
};

// the donor scan of one bucket for the point (x, y): strict <, so the first of equals stays and a NaN or infinite distance never wins
// The scan is one lane's chain of loads, each a trip to memory (few lanes of a wave are deficient): four slots at a time, their masks loaded together and then
// the coordinates of the active ones, the comparisons in slot order.
__device__ __forceinline__ void pt_nearest(const PtGeom &g, int cell, int nc, double x, double y, double &best, int &donor)
{
    int s = 0, lin = cell;
    for (; s + 4 <= g.mx; s += 4, lin += 4 * nc) {
        int m[4];
        double xs[4], ys[4];
#pragma unroll
        for (int u = 0; u < 4; u++) m[u] = g.active[lin + u * nc];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            xs[u] = ys[u] = 0.0;
            if (m[u] != 0) xs[u] = g.px[lin + u * nc], ys[u] = g.py[lin + u * nc];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (m[u] == 0) continue;
            const double ex = xs[u] - x, ey = ys[u] - y;
            const double d2 = ex * ex + ey * ey;
            if (d2 < best) best = d2, donor = lin + u * nc;
        }
    }
    for (; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        const double ex = g.px[lin] - x, ey = g.py[lin] - y;
        const double d2 = ex * ex + ey * ey;
        if (d2 < best) best = d2, donor = lin;
    }
}

// steps 2 - 7 of the definition for the deficient cell (i, j) holding n particles; it reads only slots active at entry and writes only slots inactive at entry
__device__ __forceinline__ void pt_inject_cell(const PtInjArgs &a, int i, int j, int &n, int &n_injected, int &n_no_donor)
{
    const PtGeom &g = a.g;
    const int nc = g.nx * g.ny, base = j * g.nx + i;
    const double xc = g.x0 + (double)i * g.dx, yc = g.y0 + (double)j * g.dy;
    const double fnx = (double)a.nsx, fny = (double)a.nsy;
    unsigned long long occ = 0;
    for (int s = 0, lin = base; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        const double fa = floor(((g.px[lin] - xc) * g.idx) * fnx), fb = floor(((g.py[lin] - yc) * g.idy) * fny);
        if (fa >= 0.0 && fa < fnx && fb >= 0.0 && fb < fny) occ |= 1ull << ((int)fa + a.nsx * (int)fb);
    }
    int sfree = 0, to = base;             // the lowest slot not yet looked at
    for (int qb = 0, q = 0; qb < a.nsy; qb++) {
        for (int qa = 0; qa < a.nsx; qa++, q++) {
            if (n >= a.minx) return;
            if ((occ >> q) & 1ull) continue;
            const double x = xc + ((double)qa + 0.5) * a.hx, y = yc + ((double)qb + 0.5) * a.hy;
            double best = HUGE_VAL;
            int donor = -1;
            pt_nearest(g, base, nc, x, y, best, donor);
            // the neighbour loops stay rolled: nine copies of the scan cost 36 VGPRs and a wave of occupancy on the path every thread takes
#pragma unroll 1
            for (int dj = -1; dj <= 1; dj++) {
                const int jn = j + dj;
                if (jn < 0 || jn >= g.ny) continue;
#pragma unroll 1
                for (int di = -1; di <= 1; di++) {
                    const int in = i + di;
                    if ((di == 0 && dj == 0) || in < 0 || in >= g.nx) continue;
                    pt_nearest(g, jn * g.nx + in, nc, x, y, best, donor);
                }
            }
            if (donor < 0) {
                n_no_donor = 1;
                return;
            }
            while (sfree < g.mx && g.active[to] != 0) sfree++, to += nc;
            if (sfree >= g.mx) return;    // not reached: n < min_xcell <= max_xcell leaves a slot
            g.px[to] = x, g.py[to] = y, a.aout[to] = 1;
            a.pph[to] = a.pph[donor];
#pragma unroll
            for (int k = 0; k < JRX_MAXPHASE; k++) {
                if (k >= a.nargs) continue;
                if (a.loc[k] == JRX_INJECT_DONOR) {
                    a.args[k][to] = a.args[k][donor];
                } else if (a.loc[k] == JRX_INJECT_VERTEX) {
                    const double *f = a.fields[k] + j * (g.nx + 1) + i;
                    const double f00 = f[0], f10 = f[1], f01 = f[g.nx + 1], f11 = f[g.nx + 2];
                    a.args[k][to] = pt_bilin((x - xc) * g.idx, (y - yc) * g.idy, f00, f10, f01, f11);
                } else {
                    double v;
                    if (pt_interp(a.fields[k], g.nx, g.ny, a.ox, a.oy, g.idx, g.idy, x, y, v)) a.args[k][to] = v;
                }
            }
            sfree++, to += nc;
            n++, n_injected++;
        }
    }
}

// A thread per cell.  Every thread copies its bucket's mask to the output and counts it: one coalesced read and one coalesced write per slot, the whole of the
// common path.  Only a thread whose count is below min_xcell goes on to pt_inject_cell.
__global__ __launch_bounds__(256) void k_pt_inject(const PtInjArgs a)
{
    const PtGeom &g = a.g;
    int i, j;
    pt_index(g.nx, i, j);
    int n = 0, n_before = 0, n_deficient = 0, n_injected = 0, n_no_donor = 0;
    if (i < g.nx && j < g.ny) {
        const int nc = g.nx * g.ny;
        {
            // the two masks do not overlap (checked by the entry point): four loads in flight before the four stores
            const int *__restrict__ in = g.active;
            int *__restrict__ out = a.aout;
            int s = 0, lin = j * g.nx + i;
            for (; s + 4 <= g.mx; s += 4, lin += 4 * nc) {
                const int m0 = in[lin], m1 = in[lin + nc], m2 = in[lin + 2 * nc], m3 = in[lin + 3 * nc];
                out[lin] = m0, out[lin + nc] = m1, out[lin + 2 * nc] = m2, out[lin + 3 * nc] = m3;
                n += (m0 != 0) + (m1 != 0) + (m2 != 0) + (m3 != 0);
            }
            for (; s < g.mx; s++, lin += nc) {
                const int m = in[lin];
                out[lin] = m;
                n += m != 0;
            }
        }
        n_before = n;
        if (n < a.minx) {
            n_deficient = 1;
            pt_inject_cell(a, i, j, n, n_injected, n_no_donor);
        }
    }
    // The five counts of the block, in three atomics at the most.  Every wave of every launch has particles to count, and one atomic per wave and count on one
    // cache line took longer than the copy of the mask (measured: 400 us of a 1024^2 launch).  So the waves meet in LDS, and two counts share a word: each
    // total is below 2^31 (the slots are), so the low halves never carry into the high ones.
    __shared__ int sm[kPtTY][5];
    int v[5] = {n_before, n, n_deficient, n_injected, n_no_donor};
#pragma unroll
    for (int k = 0; k < 5; k++) v[k] = pt_wave_sum(v[k]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; k++) sm[threadIdx.y][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        unsigned long long t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            int sum = 0;
#pragma unroll
            for (int r = 0; r < kPtTY; r++) sum += sm[r][k];
            t[k] = (unsigned long long)sum;
        }
        if (t[0] | t[1]) atomicAdd(a.counts + 0, t[0] | (t[1] << 32));
        if (t[2] | t[3]) atomicAdd(a.counts + 1, t[2] | (t[3] << 32));
        if (t[4]) atomicAdd(a.counts + 2, t[4]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
// jrx_particles2d as the shared checks see it (particles_common.hpp), checked, and by value for the kernels
jrx_status pt_geom(jrx_handle *h, const char *fn, const char *what, const jrx_particles2d *p, PtSet *S, PtGeom *g)
{
    *S = p ? PtSet{2, {p->px, p->py}, p->active, {p->nx, p->ny}, (int)p->max_xcell, {p->x0, p->y0}, {p->dx, p->dy}, {p->_dx, p->_dy}} : PtSet{};
    JRX_TRY(pt_check_set(h, fn, what, *S));
    *g = PtGeom{p->px, p->py, (int *)p->active, p->x0, p->y0, p->dx, p->dy, p->_dx, p->_dy, (int)p->nx, (int)p->ny, (int)p->max_xcell};
    return JRX_OK;
}

jrx_status pt_centres(jrx_handle *h, const char *fn, const PtGeom &g)
{
    if (g.nx < 2 || g.ny < 2) return jrx_fail(h, JRX_ERR_ARG, "%s: %d x %d cells (interpolation between centres needs nx >= 2 and ny >= 2)", fn, g.nx, g.ny);
    return JRX_OK;
}

jrx_status pt_method(jrx_handle *h, const char *fn, double dt, int32_t method)
{
    if (!std::isfinite(dt)) return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g (must be finite)", fn, dt);
    if (method != JRX_ROTATE_MATRIX && method != JRX_ROTATE_JAUMANN)
        return jrx_fail(h, JRX_ERR_ARG, "%s: unknown method %d (%d = matrix, %d = jaumann)", fn, (int)method, JRX_ROTATE_MATRIX, JRX_ROTATE_JAUMANN);
    return JRX_OK;
}

// One launch, counted: a thread per cell or node of the (ex, ey) box, the box whose x extent the kernel hands to pt_index.  The launchers check nothing: an entry
// point checks everything first, then launches one kernel or its chain.
template <typename K, typename... A>
void pt_launch(jrx_handle *h, K kernel, int ex, int ey, const A &...a)
{
    h->stat_particles_launches++;
    hipLaunchKernelGGL(kernel, dim3(pt_blocks(ex, ey)), dim3(kPtTX, kPtTY), 0, h->stream, a...);
}

// operators 3, 4, 6, 7 as one launch over the (nx + e, ny + e) box: e = 0, the cells; e = 1, the vertices of the F that operator 4 writes
template <typename K>
void pt_launch_field(jrx_handle *h, K kernel, int e, const PtGeom &g, const double *pF, const double *F)
{
    pt_launch(h, kernel, g.nx + e, g.ny + e, PtFieldArgs{g, (double *)pF, (double *)F, g.x0 + 0.5 * g.dx, g.y0 + 0.5 * g.dy});
}

// the entry points of operators 3, 4, 6, 7: one particle field, one grid field of extents (nx + e, ny + e)
template <typename K>
jrx_status pt_field_op(jrx_handle *h, const char *fn, K kernel, double *pF, double *F, const jrx_particles2d *part, int e, bool to_particles, bool centres)
{
    if (!h) return JRX_ERR_ARG;
    PtSet S;
    PtGeom g;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &g));
    if (centres) JRX_TRY(pt_centres(h, fn, g));
    const OpArr ap = {pF, 8 * pt_slots(S), "pF"}, af = {F, 8 * (i64)(g.nx + e) * (g.ny + e), "F"};
    JRX_TRY(to_particles ? pt_disjoint(h, fn, &ap, 1, &af, 1, S) : pt_disjoint(h, fn, &af, 1, &ap, 1, S));
    JRX_TRY(jrx_check_device(h));
    pt_launch_field(h, kernel, to_particles ? 0 : e, g, pF, F);
    return op_finish(h);
}

// fused = false: operator 8 alone on a.pxx, pyy, pxy, pw; true: the one-launch rotate_stress!
void pt_launch_rotate(jrx_handle *h, const PtRotArgs &a, int32_t method, bool fused)
{
    dispatch_const<0, 1>((int)method, [&](auto MM) {
        if (fused) pt_launch(h, k_pt_rotate_stress<MM()>, a.g.nx, a.g.ny, a);
        else pt_launch(h, k_pt_rotate<MM()>, a.g.nx, a.g.ny, a);
    });
}

// operators 10 and 11: everything checked first, then the fused launches (2 / 3) or the chain of the definition (7 launches and one fill)
jrx_status pt_subgrid(jrx_handle *h, const char *fn, bool vertex, double *pT, const double *T_grid, const double *dT_grid, int32_t dT_extent, double *pT0, double *pdT,
                      const double *pdt0, double *dT_subgrid, const jrx_particles2d *part, double d, double dt)
{
    PtSgArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    if (!vertex) JRX_TRY(pt_centres(h, fn, a.g));
    if (!(d >= 0.0 && d <= 1.0)) return jrx_fail(h, JRX_ERR_ARG, "%s: d = %g (must lie in [0, 1])", fn, d);
    if (!std::isfinite(dt) || dt < 0.0) return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g (must be finite and not negative)", fn, dt);
    if (dT_extent != JRX_SUBGRID_DT_NODES && dT_extent != JRX_SUBGRID_DT_GHOSTED)
        return jrx_fail(h, JRX_ERR_ARG, "%s: unknown ΔT extent code %d (%d = the node box, %d = one ghost layer around it)", fn, (int)dT_extent, JRX_SUBGRID_DT_NODES,
                        JRX_SUBGRID_DT_GHOSTED);
    const PtGeom &g = a.g;
    const int e = vertex ? 1 : 0, ex = g.nx + e, ey = g.ny + e, gh = dT_extent == JRX_SUBGRID_DT_GHOSTED ? 1 : 0;          // (ex, ey): the node box of the form
    const i64 ns = 8 * pt_slots(S), nn = 8 * (i64)ex * ey, nd = 8 * (i64)(ex + 2 * gh) * (ey + 2 * gh);
    const OpArr out[4] = {{pT, ns, "pT"}, {pT0, ns, "subgrid_arrays.pT0"}, {pdT, ns, "subgrid_arrays.pΔT"}, {dT_subgrid, nn, "subgrid_arrays.ΔT_subgrid"}};
    const OpArr in[3] = {{T_grid, nn, "T_grid"}, {dT_grid, nd, "ΔT_grid"}, {pdt0, ns, "subgrid_arrays.dt₀"}};
    JRX_TRY(pt_disjoint(h, fn, out, 4, in, 3, S));
    JRX_TRY(jrx_check_device(h));
    a.pT = pT, a.pT0 = pT0, a.pdT = pdT, a.pdt0 = pdt0, a.T = T_grid, a.dTg = dT_grid, a.dTs = dT_subgrid;
    a.dtn = ex + 2 * gh, a.dto = gh * (a.dtn + 1);
    a.ox = g.x0 + 0.5 * g.dx, a.oy = g.y0 + 0.5 * g.dy;
    a.ndt = (-d) * dt;
    if (h->particles_subgrid_fused) {
        if (vertex) {
            pt_launch(h, k_pt_sg_cell<true>, g.nx, g.ny, a);
            pt_launch(h, k_pt_sg_vertex, ex, ey, a);
            pt_launch(h, k_pt_sg_back<true>, g.nx, g.ny, a);
        } else {
            pt_launch(h, k_pt_sg_cell<false>, g.nx, g.ny, a);
            pt_launch(h, k_pt_sg_back<false>, g.nx, g.ny, a);
        }
        return op_finish(h);
    }
    auto to_particles = [&](double *pF, const double *F) {          // operator 3 from vertices, 6 from centres
        if (vertex) pt_launch_field(h, k_pt_grid2particle, 0, g, pF, F);
        else pt_launch_field(h, k_pt_centroid2particle, 0, g, pF, F);
    };
    pt_launch(h, k_pt_sg_copy, g.nx, g.ny, a);                                                // 1
    to_particles(pT, T_grid);                                                                 // 2
    pt_launch(h, k_pt_sg_delta, g.nx, g.ny, a);                                               // 3
    JRX_HIP(h, hipMemsetAsync(dT_subgrid, 0, (size_t)nn, h->stream));                         // 4: +0.0 is all bits zero
    if (vertex) pt_launch_field(h, k_pt_particle2grid, 1, g, pdT, dT_subgrid);
    else pt_launch_field(h, k_pt_particle2centroid, 0, g, pdT, dT_subgrid);
    pt_launch(h, k_pt_sg_remainder, ex, ey, a, ex, ey);                                       // 5
    to_particles(pdT, dT_subgrid);                                                            // 6
    pt_launch(h, k_pt_sg_add, g.nx, g.ny, a);                                                 // 7
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_particles2d_advect_rk2(jrx_handle *h, const jrx_particles2d *part, const double *Vx, const double *Vy, double dt)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "advection!(particles)";
    PtAdvArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    const PtGeom &g = a.g;
    if (!Vx || !Vy) return jrx_fail(h, JRX_ERR_ARG, "%s: V.%s is NULL", fn, !Vx ? "Vx" : "Vy");
    if (!std::isfinite(dt)) return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g (must be finite)", fn, dt);
    JRX_TRY(pt_apart(h, fn, {Vx, 8 * (i64)(g.nx + 1) * (g.ny + 2), "V.Vx"}, S));
    JRX_TRY(pt_apart(h, fn, {Vy, 8 * (i64)(g.nx + 2) * (g.ny + 1), "V.Vy"}, S));
    JRX_TRY(jrx_check_device(h));
    a.Vx = Vx, a.Vy = Vy;
    a.oyx = part->y0 - 0.5 * part->dy, a.oxy = part->x0 - 0.5 * part->dx;
    a.dt = dt, a.hdt = 0.5 * dt;
    pt_launch(h, k_pt_advect_rk2, g.nx, g.ny, a);
    return op_finish(h);
}

jrx_status jrx_particles2d_move(jrx_handle *h, const jrx_particles2d *src, const jrx_particles2d *dst, const double *const *args_src, double *const *args_dst,
                                int32_t nargs, int64_t counts[5])
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "move_particles!";
    PtMoveArgs a = {};
    PtGeom d;
    PtSet S, D;
    JRX_TRY(pt_geom(h, fn, "particles (source)", src, &S, &a.src));
    JRX_TRY(pt_geom(h, fn, "particles (destination)", dst, &D, &d));
    JRX_TRY(pt_move_checks(h, fn, S, D, args_src, args_dst, nargs, nullptr, counts));
    JRX_TRY(jrx_check_device(h));
    a.dpx = d.px, a.dpy = d.py, a.dactive = d.active;
    for (int k = 0; k < nargs; k++) a.as[k] = args_src[k], a.ad[k] = args_dst[k];
    a.nargs = (int)nargs;
    a.counts = pt_words(h);
    JRX_HIP(h, hipMemsetAsync(a.counts, 0, sizeof(int64_t) * 5, h->stream));
    pt_launch(h, k_pt_move, d.nx, d.ny, a);
    JRX_LAUNCH_CHECK(h);
    return pt_read_words(h, 0, 5, counts);
}

jrx_status jrx_particles2d_grid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles2d *part)
{
    return pt_field_op(h, "grid2particle!", k_pt_grid2particle, pF, (double *)F, part, 1, true, false);
}

jrx_status jrx_particles2d_particle2grid(jrx_handle *h, double *F, const double *pF, const jrx_particles2d *part)
{
    return pt_field_op(h, "particle2grid!", k_pt_particle2grid, (double *)pF, F, part, 1, false, false);
}

jrx_status jrx_particles2d_centroid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles2d *part)
{
    return pt_field_op(h, "centroid2particle!", k_pt_centroid2particle, pF, (double *)F, part, 0, true, true);
}

jrx_status jrx_particles2d_particle2centroid(jrx_handle *h, double *F, const double *pF, const jrx_particles2d *part)
{
    return pt_field_op(h, "particle2centroid!", k_pt_particle2centroid, (double *)pF, F, part, 0, false, false);
}

jrx_status jrx_particles2d_phase_ratios(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *pPhases, int32_t nphase,
                                        const jrx_particles2d *part, int64_t *n_empty)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "update_phase_ratios!(particles)";
    static const char *const names[4] = {"phase_ratios.center", "phase_ratios.vertex", "phase_ratios.Vx", "phase_ratios.Vy"};
    static const int stag[4][3] = {{0, 0}, {1, 1}, {1, 0}, {0, 1}};
    double *const members[4] = {center, vertex, Vx, Vy};
    PtPrArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    JRX_TRY(pt_ratio_checks(h, fn, S, members, names, stag, 4, pPhases, nphase, n_empty));
    JRX_TRY(jrx_check_device(h));
    a.center = center, a.vertex = vertex, a.Vx = Vx, a.Vy = Vy, a.pPhases = pPhases;
    a.n_empty = pt_words(h) + 5;
    JRX_HIP(h, hipMemsetAsync(a.n_empty, 0, sizeof(int64_t), h->stream));
    dispatch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)nphase, [&](auto NN) { pt_launch(h, k_pt_phase_ratios<NN()>, a.g.nx + 1, a.g.ny + 1, a); });
    JRX_LAUNCH_CHECK(h);
    return pt_read_words(h, 5, 1, n_empty);
}

jrx_status jrx_particles2d_rotate(jrx_handle *h, double *const ptau[3], const double *pomega, const jrx_particles2d *part, double dt, int32_t method)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "rotate_stress_particles!";
    PtRotArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    if (!ptau) return jrx_fail(h, JRX_ERR_ARG, "%s: ptau is NULL", fn);
    JRX_TRY(pt_method(h, fn, dt, method));
    const i64 ns = 8 * pt_slots(S);
    const OpArr out[3] = {{ptau[0], ns, "pτxx"}, {ptau[1], ns, "pτyy"}, {ptau[2], ns, "pτxy"}}, in[1] = {{pomega, ns, "pω"}};
    JRX_TRY(pt_disjoint(h, fn, out, 3, in, 1, S));
    JRX_TRY(jrx_check_device(h));
    a.pxx = ptau[0], a.pyy = ptau[1], a.pxy = ptau[2], a.pw = const_cast<double *>(pomega), a.dt = dt;
    pt_launch_rotate(h, a, method, false);
    return op_finish(h);
}

jrx_status jrx_particles2d_rotate_stress(jrx_handle *h, double *const ptau[3], double *pomega, const double *tau_xx, const double *tau_yy, const double *tau_xy,
                                         const double *omega_xy, const jrx_particles2d *part, double dt, int32_t method)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "rotate_stress!(particles)";
    PtRotArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    JRX_TRY(pt_centres(h, fn, a.g));
    if (!ptau) return jrx_fail(h, JRX_ERR_ARG, "%s: ptau is NULL", fn);
    JRX_TRY(pt_method(h, fn, dt, method));
    const PtGeom &g = a.g;
    const i64 ns = 8 * pt_slots(S), nc = 8 * (i64)g.nx * g.ny, nv = 8 * (i64)(g.nx + 1) * (g.ny + 1);
    const OpArr out[4] = {{ptau[0], ns, "pτxx"}, {ptau[1], ns, "pτyy"}, {ptau[2], ns, "pτxy"}, {pomega, ns, "pω"}};
    const OpArr in[4] = {{tau_xx, nc, "τ.xx"}, {tau_yy, nc, "τ.yy"}, {tau_xy, nv, "τ.xy"}, {omega_xy, nv, "ω.xy"}};
    JRX_TRY(pt_disjoint(h, fn, out, 4, in, 4, S));
    JRX_TRY(jrx_check_device(h));
    a.pxx = ptau[0], a.pyy = ptau[1], a.pxy = ptau[2], a.pw = pomega, a.dt = dt;
    if (h->particles_stress_fused) {
        a.txx = tau_xx, a.tyy = tau_yy, a.txy = tau_xy, a.wxy = omega_xy;
        a.ox = g.x0 + 0.5 * g.dx, a.oy = g.y0 + 0.5 * g.dy;
        pt_launch_rotate(h, a, method, true);
    } else {
        pt_launch_field(h, k_pt_centroid2particle, 0, g, ptau[0], tau_xx);
        pt_launch_field(h, k_pt_centroid2particle, 0, g, ptau[1], tau_yy);
        pt_launch_field(h, k_pt_grid2particle, 0, g, ptau[2], tau_xy);
        pt_launch_field(h, k_pt_grid2particle, 0, g, pomega, omega_xy);
        pt_launch_rotate(h, a, method, false);
    }
    return op_finish(h);
}

jrx_status jrx_particles2d_stress2grid(jrx_handle *h, double *const tau_o[6], const double *const ptau[3], const jrx_particles2d *part)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "stress2grid!";
    PtS2GArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    if (!tau_o || !ptau) return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL", fn, !tau_o ? "tau_o" : "ptau");
    const PtGeom &g = a.g;
    const i64 ns = 8 * pt_slots(S), nc = 8 * (i64)g.nx * g.ny, nv = 8 * (i64)(g.nx + 1) * (g.ny + 1);
    const OpArr out[6] = {{tau_o[0], nc, "τ_o.xx"}, {tau_o[1], nc, "τ_o.yy"}, {tau_o[2], nc, "τ_o.xy_c"}, {tau_o[3], nv, "τ_o.xy"}, {tau_o[4], nv, "τ_o.xx_v"},
                          {tau_o[5], nv, "τ_o.yy_v"}};
    const OpArr in[3] = {{ptau[0], ns, "pτxx"}, {ptau[1], ns, "pτyy"}, {ptau[2], ns, "pτxy"}};
    JRX_TRY(pt_disjoint(h, fn, out, 6, in, 3, S));
    JRX_TRY(jrx_check_device(h));
    if (h->particles_stress_fused) {
        a.cxx = tau_o[0], a.cyy = tau_o[1], a.cxy = tau_o[2], a.vxy = tau_o[3], a.vxx = tau_o[4], a.vyy = tau_o[5];
        a.pxx = ptau[0], a.pyy = ptau[1], a.pxy = ptau[2];
        pt_launch(h, k_pt_stress2grid, g.nx + 1, g.ny + 1, a);
    } else {
        for (int c = 0; c < 3; c++) pt_launch_field(h, k_pt_particle2centroid, 0, g, ptau[c], tau_o[c]);          // xx, yy, xy_c
        pt_launch_field(h, k_pt_particle2grid, 1, g, ptau[0], tau_o[4]);                                          // xx_v, yy_v, xy
        pt_launch_field(h, k_pt_particle2grid, 1, g, ptau[1], tau_o[5]);
        pt_launch_field(h, k_pt_particle2grid, 1, g, ptau[2], tau_o[3]);
    }
    return op_finish(h);
}

jrx_status jrx_particles2d_subgrid_diffusion_centroid(jrx_handle *h, double *pT, const double *T_grid, const double *dT_grid, int32_t dT_extent, double *pT0,
                                                      double *pdT, const double *pdt0, double *dT_subgrid, const jrx_particles2d *part, double d, double dt)
{
    if (!h) return JRX_ERR_ARG;
    return pt_subgrid(h, "subgrid_diffusion_centroid!", false, pT, T_grid, dT_grid, dT_extent, pT0, pdT, pdt0, dT_subgrid, part, d, dt);
}

jrx_status jrx_particles2d_subgrid_diffusion_vertex(jrx_handle *h, double *pT, const double *T_grid, const double *dT_grid, int32_t dT_extent, double *pT0, double *pdT,
                                                    const double *pdt0, double *dT_subgrid, const jrx_particles2d *part, double d, double dt)
{
    if (!h) return JRX_ERR_ARG;
    return pt_subgrid(h, "subgrid_diffusion!", true, pT, T_grid, dT_grid, dT_extent, pT0, pdT, pdt0, dT_subgrid, part, d, dt);
}

jrx_status jrx_particles2d_inject(jrx_handle *h, const jrx_particles2d *part, int32_t *active_out, double *pPhases, double *const *args, const double *const *fields,
                                  const int32_t *field_loc, int32_t nargs, int32_t min_xcell, int32_t nsx, int32_t nsy, int64_t counts[5])
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "inject_particles_phase!";
    PtInjArgs a = {};
    PtSet S;
    JRX_TRY(pt_geom(h, fn, "particles", part, &S, &a.g));
    const PtGeom &g = a.g;
    if (!active_out || !pPhases || !counts) return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL", fn, !active_out ? "active_out" : (!pPhases ? "pPhases" : "counts"));
    if (nsx < 1 || nsy < 1 || (i64)nsx * nsy > 64)
        return jrx_fail(h, JRX_ERR_ARG, "%s: a lattice of %d x %d sub-cells (both must be >= 1 and their product <= 64)", fn, (int)nsx, (int)nsy);
    if (min_xcell < 1 || min_xcell > g.mx || min_xcell > nsx * nsy)
        return jrx_fail(h, JRX_ERR_ARG, "%s: min_xcell = %d (must lie in 1 .. min(max_xcell = %d, nsx nsy = %d))", fn, (int)min_xcell, g.mx, (int)(nsx * nsy));
    if (nargs < 0 || nargs > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d particle fields (0 .. %d are built)", fn, (int)nargs, JRX_MAXPHASE);
    if (nargs > 0 && (!args || !fields || !field_loc))
        return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL with %d particle fields", fn, !args ? "args" : (!fields ? "fields" : "field_loc"), (int)nargs);
    for (int k = 0; k < nargs; k++) {
        const int loc = field_loc[k];
        if (loc != JRX_INJECT_VERTEX && loc != JRX_INJECT_CENTRE && loc != JRX_INJECT_DONOR)
            return jrx_fail(h, JRX_ERR_ARG, "%s: unknown field_loc %d of particle field %d (%d = vertex, %d = centre, %d = donor)", fn, loc, k + 1, JRX_INJECT_VERTEX,
                            JRX_INJECT_CENTRE, JRX_INJECT_DONOR);
        if (!args[k]) return jrx_fail(h, JRX_ERR_ARG, "%s: particle field %d is NULL", fn, k + 1);
        if (loc != JRX_INJECT_DONOR && !fields[k]) return jrx_fail(h, JRX_ERR_ARG, "%s: grid field %d is NULL", fn, k + 1);
        if (loc == JRX_INJECT_CENTRE) JRX_TRY(pt_centres(h, fn, g));
    }
    // everything written -- the mask's copy, the phases, the particle fields, and the coordinates in place -- apart from the mask that is read and from each other
    const i64 ns = pt_slots(S);
    if (op_overlaps(active_out, 4 * ns, g.active, 4 * ns)) return jrx_fail(h, JRX_ERR_ARG, "%s: active_out overlaps the mask (the mask is written out of place)", fn);
    OpArr out[2 + JRX_MAXPHASE] = {{active_out, 4 * ns, "active_out"}, {pPhases, 8 * ns, "pPhases"}};
    static const char *const names[JRX_MAXPHASE] = {"particle field 1", "particle field 2", "particle field 3", "particle field 4",
                                                    "particle field 5", "particle field 6", "particle field 7", "particle field 8"};
    for (int k = 0; k < nargs; k++) out[2 + k] = OpArr{args[k], 8 * ns, names[k]};
    OpArr in[JRX_MAXPHASE];
    int nin = 0;
    for (int k = 0; k < nargs; k++) {
        if (field_loc[k] == JRX_INJECT_DONOR) continue;
        const bool v = field_loc[k] == JRX_INJECT_VERTEX;
        in[nin++] = OpArr{fields[k], 8 * (i64)(g.nx + (v ? 1 : 0)) * (g.ny + (v ? 1 : 0)), v ? "a vertex field" : "a centre field"};
    }
    JRX_TRY(pt_disjoint(h, fn, out, 2 + nargs, in, nin, S));
    for (int k = 0; k < nin; k++) JRX_TRY(pt_apart(h, fn, in[k], S));          // px, py are written too
    JRX_TRY(jrx_check_device(h));
    a.aout = (int *)active_out, a.pph = pPhases;
    for (int k = 0; k < nargs; k++) a.args[k] = args[k], a.fields[k] = fields[k], a.loc[k] = field_loc[k];
    a.nargs = (int)nargs, a.minx = (int)min_xcell, a.nsx = (int)nsx, a.nsy = (int)nsy;
    a.hx = g.dx / (double)nsx, a.hy = g.dy / (double)nsy;
    a.ox = g.x0 + 0.5 * g.dx, a.oy = g.y0 + 0.5 * g.dy;
    a.counts = pt_words(h);
    JRX_HIP(h, hipMemsetAsync(a.counts, 0, sizeof(int64_t) * 3, h->stream));
    pt_launch(h, k_pt_inject, g.nx, g.ny, a);
    JRX_LAUNCH_CHECK(h);
    int64_t w[3];
    JRX_TRY(pt_read_words(h, 0, 3, w));
    const int64_t lo = 0xffffffffll;
    counts[0] = w[0] & lo, counts[1] = (w[0] >> 32) & lo, counts[2] = w[1] & lo, counts[3] = (w[1] >> 32) & lo, counts[4] = w[2];
    return JRX_OK;
}

}  // extern "C"
