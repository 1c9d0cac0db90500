// particles3d.hip -- 3D marker-in-cell particles in gather form: advection!(particles, RungeKutta2(), V, dt), move_particles!, grid2particle!, particle2grid!,
// update_phase_ratios!(phase_ratios, particles, pPhases), centroid2particle! and particle2centroid! for gfx950 -- the chain the reference's 3D miniapps take from
// JustPIC (miniapps/benchmarks/stokes3D/shear_heating/Shearheating3D.jl:63-78,224-233).  JustPIC's text is not in the reference tree: include/jrx.h (section
// "3D marker-in-cell particles") states the definitions built here, tests/_particles3d.py is the same text in NumPy.
//
// A file of its own beside particles.hip: the 2D file already holds twelve operators, and nothing of its kernels carries over but the per-axis helpers.  Those, and
// the whole host check layer (the checks of a particle set, the overlap rules, the checks of move and of the phase ratios, the counter read-back), both files take
// from particles_common.hpp; here are the kernels, the conversion of jrx_particles3d (p3_geom), the launches and the entry points.
//
// Layout: every per-particle array is (nx, ny, nz, max_xcell) column-major, the slot index slowest.  A block is 64 x 2 x 2 threads, a thread owns a cell (or a
// node) and walks the slots: in every trip of a slot loop the 64 lanes of a wave read 64 consecutive addresses.  An inactive slot holds 0 everywhere.
//
// As in 2D every kernel is a gather (a thread writes only what it owns, every loop is bounded by max_xcell or a constant), the only atomics are integer adds of
// per-wave counts into the counter words, fp64 without fma, and an index derived from a coordinate is range-checked on the double before the conversion.
// Addressing: 32-bit element offsets into the particle arrays (nx ny nz max_xcell < 2^31, checked) and into the grid fields ((nx+2)(ny+2)(nz+2) < 2^31, checked).
//
// move has two forms that leave the same bits.  Direct: a destination cell walks the slots of its 27 source cells and computes the owner of every particle from
// its three coordinates -- every coordinate is requested 27 times.  Codes: a pre-pass, a thread per source cell, stores each slot's owner as one byte (the
// neighbour offset 0 .. 26, or inactive / outside / far) and takes the three loss counters; the gather then reads 27 bytes per slot and loads coordinates and
// fields only of the slots it takes.
#include "particles_common.hpp"

namespace {

constexpr int kP3TX = 64, kP3TY = 2, kP3TZ = 2;       // block of cells / nodes: 64 x 2 x 2

struct P3Geom {                                       // jrx_particles3d by value, 32-bit extents
    double *px, *py, *pz;
    int *active;
    double x0, y0, z0, dx, dy, dz, idx, idy, idz;
    int nx, ny, nz, mx;                               // mx = max_xcell
};

__device__ __forceinline__ void p3_index(int &i, int &j, int &k)
{
    i = (int)blockIdx.x * kP3TX + (int)threadIdx.x;
    j = (int)blockIdx.y * kP3TY + (int)threadIdx.y;
    k = (int)blockIdx.z * kP3TZ + (int)threadIdx.z;
}

// the trilinear form: the bilinear form on the planes k0 and k0 + 1, then along z
__device__ __forceinline__ double p3_trilin(double tx, double ty, double tz, const double (&v)[8])
{
    return (1.0 - tz) * pt_bilin(tx, ty, v[0], v[1], v[2], v[3]) + tz * pt_bilin(tx, ty, v[4], v[5], v[6], v[7]);
}

// the eight nodes of the cell at p in an array whose rows are mx long and whose planes hold mxy entries
__device__ __forceinline__ void p3_load8(const double *__restrict__ p, int mx, int mxy, double (&v)[8])
{
    v[0] = p[0], v[1] = p[1], v[2] = p[mx], v[3] = p[mx + 1];
    v[4] = p[mxy], v[5] = p[mxy + 1], v[6] = p[mxy + mx], v[7] = p[mxy + mx + 1];
}

// one component A of extents (mx, my, mz), node grid origin (ox, oy, oz), at (x, y, z); false (and no load) when a scaled coordinate is not finite
__device__ __forceinline__ bool p3_interp(const double *__restrict__ A, int mx, int my, int mz, double ox, double oy, double oz, const P3Geom &g, double x, double y,
                                          double z, double &out)
{
    const double sx = (x - ox) * g.idx, sy = (y - oy) * g.idy, sz = (z - oz) * g.idz;
    if (!pt_finite(sx) || !pt_finite(sy) || !pt_finite(sz)) return false;
    const int i0 = pt_pair(sx, mx), j0 = pt_pair(sy, my), k0 = pt_pair(sz, mz);
    const double tx = sx - (double)i0, ty = sy - (double)j0, tz = sz - (double)k0;
    double v[8];
    p3_load8(A + ((k0 * my + j0) * mx + i0), mx, mx * my, v);
    out = p3_trilin(tx, ty, tz, v);
    return true;
}

// ------------------------------------------------------------------------------------------------ 1. advection, midpoint rule
struct P3AdvArgs {
    P3Geom g;
    const double *Vx, *Vy, *Vz;
    double hx, hy, hz;        // the ghost origins x0 - 0.5 dx, y0 - 0.5 dy, z0 - 0.5 dz
    double dt, hdt;
};

__device__ __forceinline__ bool p3_velocity(const P3AdvArgs &a, double x, double y, double z, double &ux, double &uy, double &uz)
{
    const P3Geom &g = a.g;
    return p3_interp(a.Vx, g.nx + 1, g.ny + 2, g.nz + 2, g.x0, a.hy, a.hz, g, x, y, z, ux) &&
           p3_interp(a.Vy, g.nx + 2, g.ny + 1, g.nz + 2, a.hx, g.y0, a.hz, g, x, y, z, uy) &&
           p3_interp(a.Vz, g.nx + 2, g.ny + 2, g.nz + 1, a.hx, a.hy, g.z0, g, x, y, z, uz);
}

__global__ __launch_bounds__(256) void k_p3_advect_rk2(const P3AdvArgs a)
{
    const P3Geom &g = a.g;
    int i, j, k;
    p3_index(i, j, k);
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;
    const int nc = g.nx * g.ny * g.nz;
    int lin = (k * g.ny + j) * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        const double x = g.px[lin], y = g.py[lin], z = g.pz[lin];
        double ux, uy, uz, wx, wy, wz;
        if (!p3_velocity(a, x, y, z, ux, uy, uz)) continue;
        const double xm = x + a.hdt * ux, ym = y + a.hdt * uy, zm = z + a.hdt * uz;
        if (!p3_velocity(a, xm, ym, zm, wx, wy, wz)) continue;
        g.px[lin] = x + a.dt * wx;
        g.py[lin] = y + a.dt * wy;
        g.pz[lin] = z + a.dt * wz;
    }
}

// ------------------------------------------------------------------------------------------------ 2. move: a destination cell gathers its particles
struct P3MoveArgs {
    P3Geom src;
    double *dpx, *dpy, *dpz;
    int *dactive;
    const double *as[JRX_MAXPHASE];
    double *ad[JRX_MAXPHASE];
    int nargs;
    unsigned char *codes;            // the codes form: one byte per slot, laid out as the particle arrays
    unsigned long long *counts;      // n_active_before, n_active_after, n_outside, n_far, n_overflow
};

constexpr int kP3Stay = 13;                                  // the code of the offset (0, 0, 0): (dk + 1) 9 + (dj + 1) 3 + (di + 1)
constexpr int kP3Inactive = 255, kP3Outside = 254, kP3Far = 253;

// owner cell of (x, y, z): false outside the grid
__device__ __forceinline__ bool p3_owner(const P3Geom &g, double x, double y, double z, int &ic, int &jc, int &kc)
{
    const double fx = floor((x - g.x0) * g.idx), fy = floor((y - g.y0) * g.idy), fz = floor((z - g.z0) * g.idz);
    if (!(fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny && fz >= 0.0 && fz < (double)g.nz)) return false;
    ic = (int)fx, jc = (int)fy, kc = (int)fz;
    return true;
}

__device__ __forceinline__ void p3_place(const P3MoveArgs &a, int from, int to, double x, double y, double z)
{
    a.dpx[to] = x, a.dpy[to] = y, a.dpz[to] = z, a.dactive[to] = 1;
#pragma unroll
    for (int q = 0; q < JRX_MAXPHASE; q++)
        if (q < a.nargs) a.ad[q][to] = a.as[q][from];
}

__device__ __forceinline__ void p3_clear(const P3MoveArgs &a, int n, int base, int nc)
{
    for (int s = n, to = base + n * nc; s < a.src.mx; s++, to += nc) {
        a.dpx[to] = 0.0, a.dpy[to] = 0.0, a.dpz[to] = 0.0, a.dactive[to] = 0;
#pragma unroll
        for (int q = 0; q < JRX_MAXPHASE; q++)
            if (q < a.nargs) a.ad[q][to] = 0.0;
    }
}

// the direct form: the 2D kernel's structure over 27 cells
__global__ __launch_bounds__(256) void k_p3_move(const P3MoveArgs a)
{
    const P3Geom &g = a.src;
    int i, j, k;
    p3_index(i, j, k);
    const bool live = i < g.nx && j < g.ny && k < g.nz;
    const int nc = g.nx * g.ny * g.nz, mx = g.mx;
    int n = 0, n_before = 0, n_outside = 0, n_far = 0, n_overflow = 0;
    if (live) {
        const int base = (k * g.ny + j) * g.nx + i;
        // the cell's own particles first: they always fit
        for (int s = 0, lin = base; s < mx; s++, lin += nc) {
            if (g.active[lin] == 0) continue;
            n_before++;
            const double x = g.px[lin], y = g.py[lin], z = g.pz[lin];
            int ic, jc, kc;
            if (!p3_owner(g, x, y, z, ic, jc, kc)) { n_outside++; continue; }
            const int di = ic - i, dj = jc - j, dk = kc - k;
            if (di < -1 || di > 1 || dj < -1 || dj > 1 || dk < -1 || dk > 1) { n_far++; continue; }
            if (di == 0 && dj == 0 && dk == 0) {
                p3_place(a, lin, base + n * nc, x, y, z);
                n++;
            }
        }
        // then the 26 neighbours, dk outermost; the loops stay rolled: 26 copies of the slot loop buy nothing
#pragma unroll 1
        for (int dk = -1; dk <= 1; dk++) {
            const int kn = k + dk;
            if (kn < 0 || kn >= g.nz) continue;
#pragma unroll 1
            for (int dj = -1; dj <= 1; dj++) {
                const int jn = j + dj;
                if (jn < 0 || jn >= g.ny) continue;
#pragma unroll 1
                for (int di = -1; di <= 1; di++) {
                    const int in = i + di;
                    if ((di == 0 && dj == 0 && dk == 0) || in < 0 || in >= g.nx) continue;
                    for (int s = 0, lin = (kn * g.ny + jn) * g.nx + in; s < mx; s++, lin += nc) {
                        if (g.active[lin] == 0) continue;
                        const double x = g.px[lin], y = g.py[lin], z = g.pz[lin];
                        int ic, jc, kc;
                        if (!p3_owner(g, x, y, z, ic, jc, kc) || ic != i || jc != j || kc != k) continue;
                        if (n < mx) {
                            p3_place(a, lin, base + n * nc, x, y, z);
                            n++;
                        } else {
                            n_overflow++;
                        }
                    }
                }
            }
        }
        p3_clear(a, n, base, nc);
    }
    pt_count(a.counts + 0, n_before);
    pt_count(a.counts + 1, n);
    pt_count(a.counts + 2, n_outside);
    pt_count(a.counts + 3, n_far);
    pt_count(a.counts + 4, n_overflow);
}

// the codes form, pre-pass: a thread per source cell writes one byte per slot and takes the three loss counters
__global__ __launch_bounds__(256) void k_p3_move_codes(const P3MoveArgs a)
{
    const P3Geom &g = a.src;
    int i, j, k;
    p3_index(i, j, k);
    const bool live = i < g.nx && j < g.ny && k < g.nz;
    const int nc = g.nx * g.ny * g.nz;
    int n_before = 0, n_outside = 0, n_far = 0;
    if (live) {
        int lin = (k * g.ny + j) * g.nx + i;
        for (int s = 0; s < g.mx; s++, lin += nc) {
            int code = kP3Inactive;
            if (g.active[lin] != 0) {
                n_before++;
                int ic, jc, kc;
                if (!p3_owner(g, g.px[lin], g.py[lin], g.pz[lin], ic, jc, kc)) {
                    code = kP3Outside, n_outside++;
                } else {
                    const int di = ic - i, dj = jc - j, dk = kc - k;
                    if (di < -1 || di > 1 || dj < -1 || dj > 1 || dk < -1 || dk > 1) code = kP3Far, n_far++;
                    else code = (dk + 1) * 9 + (dj + 1) * 3 + (di + 1);
                }
            }
            a.codes[lin] = (unsigned char)code;
        }
    }
    pt_count(a.counts + 0, n_before);
    pt_count(a.counts + 2, n_outside);
    pt_count(a.counts + 3, n_far);
}

// the codes form, gather: a particle of the source cell at offset (di, dj, dk) belongs here when its code names the opposite offset, 26 - code(di, dj, dk)
__global__ __launch_bounds__(256) void k_p3_move_gather(const P3MoveArgs a)
{
    const P3Geom &g = a.src;
    int i, j, k;
    p3_index(i, j, k);
    const bool live = i < g.nx && j < g.ny && k < g.nz;
    const int nc = g.nx * g.ny * g.nz, mx = g.mx;
    int n = 0, n_overflow = 0;
    if (live) {
        const int base = (k * g.ny + j) * g.nx + i;
        for (int s = 0, lin = base; s < mx; s++, lin += nc) {
            if (a.codes[lin] != kP3Stay) continue;
            p3_place(a, lin, base + n * nc, g.px[lin], g.py[lin], g.pz[lin]);
            n++;
        }
#pragma unroll 1
        for (int dk = -1; dk <= 1; dk++) {
            const int kn = k + dk;
            if (kn < 0 || kn >= g.nz) continue;
#pragma unroll 1
            for (int dj = -1; dj <= 1; dj++) {
                const int jn = j + dj;
                if (jn < 0 || jn >= g.ny) continue;
#pragma unroll 1
                for (int di = -1; di <= 1; di++) {
                    const int in = i + di;
                    if ((di == 0 && dj == 0 && dk == 0) || in < 0 || in >= g.nx) continue;
                    const int mine = 26 - ((dk + 1) * 9 + (dj + 1) * 3 + (di + 1));
                    for (int s = 0, lin = (kn * g.ny + jn) * g.nx + in; s < mx; s++, lin += nc) {
                        if (a.codes[lin] != mine) continue;
                        if (n < mx) {
                            p3_place(a, lin, base + n * nc, g.px[lin], g.py[lin], g.pz[lin]);
                            n++;
                        } else {
                            n_overflow++;
                        }
                    }
                }
            }
        }
        p3_clear(a, n, base, nc);
    }
    pt_count(a.counts + 1, n);
    pt_count(a.counts + 4, n_overflow);
}

// ------------------------------------------------------------------------------------------------ 3. grid2particle
struct P3FieldArgs {          // a particle field and a grid field: which is written depends on the operator
    P3Geom g;
    double *pF;
    double *F;
    double ox, oy, oz;        // operator 6: origin of the centre nodes
};

__global__ __launch_bounds__(256) void k_p3_grid2particle(const P3FieldArgs a)
{
    const P3Geom &g = a.g;
    int i, j, k;
    p3_index(i, j, k);
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;
    const int nc = g.nx * g.ny * g.nz, vx = g.nx + 1, vxy = (g.nx + 1) * (g.ny + 1);
    double f[8];
    p3_load8(a.F + (k * vxy + j * vx + i), vx, vxy, f);
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy, zv = g.z0 + (double)k * g.dz;
    int lin = (k * g.ny + j) * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        double v = 0.0;
        if (g.active[lin] != 0) v = p3_trilin((g.px[lin] - xv) * g.idx, (g.py[lin] - yv) * g.idy, (g.pz[lin] - zv) * g.idz, f);
        a.pF[lin] = v;
    }
}

// ------------------------------------------------------------------------------------------------ 4. particle2grid
__global__ __launch_bounds__(256) void k_p3_particle2grid(const P3FieldArgs a)
{
    const P3Geom &g = a.g;
    int i, j, k;
    p3_index(i, j, k);
    if (i > g.nx || j > g.ny || k > g.nz) return;
    const int nc = g.nx * g.ny * g.nz;
    const double xv = g.x0 + (double)i * g.dx, yv = g.y0 + (double)j * g.dy, zv = g.z0 + (double)k * g.dz;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int oi = -1; oi <= 0; oi++) {
#pragma unroll
        for (int oj = -1; oj <= 0; oj++) {
#pragma unroll
            for (int ok = -1; ok <= 0; ok++) {
                const int ic = i + oi, jc = j + oj, kc = k + ok;
                if (ic < 0 || ic >= g.nx || jc < 0 || jc >= g.ny || kc < 0 || kc >= g.nz) continue;
                for (int s = 0, lin = (kc * g.ny + jc) * g.nx + ic; s < g.mx; s++, lin += nc) {
                    if (g.active[lin] == 0) continue;
                    const double w = pt_w(g.px[lin], xv, g.idx) * pt_w(g.py[lin], yv, g.idy) * pt_w(g.pz[lin], zv, g.idz);
                    num += w * a.pF[lin];
                    den += w;
                }
            }
        }
    }
    if (!(den == 0.0)) a.F[(k * (g.ny + 1) + j) * (g.nx + 1) + i] = num / den;
}

// ------------------------------------------------------------------------------------------------ 5. phase ratios
constexpr int kP3Members = 8;
// the stagger (sx, sy, sz) of center, vertex, Vx, Vy, Vz, yz, xz, xy
__device__ constexpr int kP3Stag[kP3Members][3] = {{0, 0, 0}, {1, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};

struct P3PrArgs {
    P3Geom g;
    double *out[kP3Members];
    const double *pPhases;
    unsigned long long *n_empty;
};

template <int N>
__device__ __forceinline__ void p3_add(double (&acc)[N], double &W, int k, double w)
{
#pragma unroll
    for (int q = 0; q < N; q++) acc[q] = q == k ? acc[q] + w : acc[q];
    W += w;
}

// One walk of the node's eight cells feeds the members of MASK (bit m = member m); a launch with all eight bits, or two launches with four each.  A cell at
// offset (oi, oj, ok) feeds a member when its offset is 0 along every axis the member is not staggered on: compile-time after unrolling, so the accumulators
// stay in registers, and each member sees its cells in the nesting order of (4).
template <int N, int MASK>
__global__ __launch_bounds__(256) void k_p3_phase_ratios(const P3PrArgs a)
{
    const P3Geom &g = a.g;
    int i, j, k;
    p3_index(i, j, k);
    const bool live = i <= g.nx && j <= g.ny && k <= g.nz;
    int empty = 0;
    if (live) {
        const int nc = g.nx * g.ny * g.nz;
        // [0]: the centre coordinate, [1]: the vertex coordinate
        const double xn[2] = {g.x0 + ((double)i + 0.5) * g.dx, g.x0 + (double)i * g.dx};
        const double yn[2] = {g.y0 + ((double)j + 0.5) * g.dy, g.y0 + (double)j * g.dy};
        const double zn[2] = {g.z0 + ((double)k + 0.5) * g.dz, g.z0 + (double)k * g.dz};
        double acc[kP3Members][N], W[kP3Members];
#pragma unroll
        for (int m = 0; m < kP3Members; m++) {
            W[m] = 0.0;
#pragma unroll
            for (int q = 0; q < N; q++) acc[m][q] = 0.0;
        }
#pragma unroll
        for (int oi = -1; oi <= 0; oi++) {
#pragma unroll
            for (int oj = -1; oj <= 0; oj++) {
#pragma unroll
                for (int ok = -1; ok <= 0; ok++) {
                    bool fed = false;          // does this cell feed a member of MASK at all?
#pragma unroll
                    for (int m = 0; m < kP3Members; m++)
                        if (((MASK >> m) & 1) && (kP3Stag[m][0] || oi == 0) && (kP3Stag[m][1] || oj == 0) && (kP3Stag[m][2] || ok == 0)) fed = true;
                    if (!fed) continue;
                    const int ic = i + oi, jc = j + oj, kc = k + ok;
                    if (ic < 0 || ic >= g.nx || jc < 0 || jc >= g.ny || kc < 0 || kc >= g.nz) continue;
                    for (int s = 0, lin = (kc * g.ny + jc) * g.nx + ic; s < g.mx; s++, lin += nc) {
                        if (g.active[lin] == 0) continue;
                        const double p = a.pPhases[lin];
                        if (!(p >= 1.0 && p < (double)(N + 1))) continue;
                        const int ph = (int)p - 1;
                        const double x = g.px[lin], y = g.py[lin], z = g.pz[lin];
                        const double wx[2] = {pt_w(x, xn[0], g.idx), pt_w(x, xn[1], g.idx)};
                        const double wy[2] = {pt_w(y, yn[0], g.idy), pt_w(y, yn[1], g.idy)};
                        const double wz[2] = {pt_w(z, zn[0], g.idz), pt_w(z, zn[1], g.idz)};
#pragma unroll
                        for (int m = 0; m < kP3Members; m++) {
                            const int sx = kP3Stag[m][0], sy = kP3Stag[m][1], sz = kP3Stag[m][2];
                            if (((MASK >> m) & 1) && (sx || oi == 0) && (sy || oj == 0) && (sz || ok == 0)) p3_add<N>(acc[m], W[m], ph, wx[sx] * wy[sy] * wz[sz]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < kP3Members; m++) {
            if (!((MASK >> m) & 1)) continue;
            const int ex = g.nx + kP3Stag[m][0], ey = g.ny + kP3Stag[m][1], ez = g.nz + kP3Stag[m][2];
            if (i >= ex || j >= ey || k >= ez) continue;
            if (W[m] == 0.0) {
                empty++;
                continue;
            }
            double *__restrict__ out = a.out[m] + (size_t)((k * ey + j) * ex + i) * N;
#pragma unroll
            for (int q = 0; q < N; q++) out[q] = acc[m][q] / W[m];
        }
    }
    pt_count(a.n_empty, empty);
}

// ------------------------------------------------------------------------------------------------ 6. centroid2particle
__global__ __launch_bounds__(256) void k_p3_centroid2particle(const P3FieldArgs a)
{
    const P3Geom &g = a.g;
    int i, j, k;
    p3_index(i, j, k);
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;
    const int nc = g.nx * g.ny * g.nz;
    int lin = (k * g.ny + j) * g.nx + i;
    for (int s = 0; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) {
            a.pF[lin] = 0.0;
            continue;
        }
        double v;
        if (p3_interp(a.F, g.nx, g.ny, g.nz, a.ox, a.oy, a.oz, g, g.px[lin], g.py[lin], g.pz[lin], v)) a.pF[lin] = v;
    }
}

// ------------------------------------------------------------------------------------------------ 7. particle2centroid
__global__ __launch_bounds__(256) void k_p3_particle2centroid(const P3FieldArgs a)
{
    const P3Geom &g = a.g;
    int i, j, k;
    p3_index(i, j, k);
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;
    const int nc = g.nx * g.ny * g.nz, cell = (k * g.ny + j) * g.nx + i;
    const double xc = g.x0 + ((double)i + 0.5) * g.dx, yc = g.y0 + ((double)j + 0.5) * g.dy, zc = g.z0 + ((double)k + 0.5) * g.dz;
    double num = 0.0, den = 0.0;
    for (int s = 0, lin = cell; s < g.mx; s++, lin += nc) {
        if (g.active[lin] == 0) continue;
        const double w = pt_w(g.px[lin], xc, g.idx) * pt_w(g.py[lin], yc, g.idy) * pt_w(g.pz[lin], zc, g.idz);
        num += w * a.pF[lin];
        den += w;
    }
    if (!(den == 0.0)) a.F[cell] = num / den;
}

// ------------------------------------------------------------------------------------------------ host side
// jrx_particles3d as the shared checks see it (particles_common.hpp), checked, and by value for the kernels
jrx_status p3_geom(jrx_handle *h, const char *fn, const char *what, const jrx_particles3d *p, PtSet *S, P3Geom *g)
{
    *S = p ? PtSet{3, {p->px, p->py, p->pz}, p->active, {p->nx, p->ny, p->nz}, (int)p->max_xcell, {p->x0, p->y0, p->z0}, {p->dx, p->dy, p->dz}, {p->_dx, p->_dy, p->_dz}}
           : PtSet{};
    JRX_TRY(pt_check_set(h, fn, what, *S));
    *g = P3Geom{p->px, p->py, p->pz, (int *)p->active, p->x0, p->y0, p->z0, p->dx, p->dy, p->dz, p->_dx, p->_dy, p->_dz, (int)p->nx, (int)p->ny, (int)p->nz,
                (int)p->max_xcell};
    return JRX_OK;
}

dim3 p3_grid(int ex, int ey, int ez) { return dim3((ex + kP3TX - 1) / kP3TX, (ey + kP3TY - 1) / kP3TY, (ez + kP3TZ - 1) / kP3TZ); }
const dim3 kP3Block(kP3TX, kP3TY, kP3TZ);

// operators 3, 4, 6, 7: one particle field, one grid field of extents (nx + e, ny + e, nz + e)
template <typename K>
jrx_status p3_field_op(jrx_handle *h, const char *fn, K kernel, double *pF, double *F, const jrx_particles3d *part, int e, bool to_particles, bool centres)
{
    if (!h) return JRX_ERR_ARG;
    P3FieldArgs a = {};
    PtSet S;
    JRX_TRY(p3_geom(h, fn, "particles", part, &S, &a.g));
    const P3Geom &g = a.g;
    if (centres && (g.nx < 2 || g.ny < 2 || g.nz < 2))
        return jrx_fail(h, JRX_ERR_ARG, "%s: %d x %d x %d cells (interpolation between centres needs every extent >= 2)", fn, g.nx, g.ny, g.nz);
    const OpArr ap = {pF, 8 * pt_slots(S), "pF"}, af = {F, 8 * (i64)(g.nx + e) * (g.ny + e) * (g.nz + e), "F"};
    JRX_TRY(to_particles ? pt_disjoint(h, fn, &ap, 1, &af, 1, S) : pt_disjoint(h, fn, &af, 1, &ap, 1, S));
    JRX_TRY(jrx_check_device(h));
    a.pF = pF, a.F = F;
    a.ox = g.x0 + 0.5 * g.dx, a.oy = g.y0 + 0.5 * g.dy, a.oz = g.z0 + 0.5 * g.dz;
    const int n = to_particles ? 0 : e;          // a thread per cell, or per node of the field that is written
    h->stat_particles_launches++;
    hipLaunchKernelGGL(kernel, p3_grid(g.nx + n, g.ny + n, g.nz + n), kP3Block, 0, h->stream, a);
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_particles3d_advect_rk2(jrx_handle *h, const jrx_particles3d *part, const double *Vx, const double *Vy, const double *Vz, double dt)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "advection!(particles)";
    P3AdvArgs a = {};
    PtSet S;
    JRX_TRY(p3_geom(h, fn, "particles", part, &S, &a.g));
    const P3Geom &g = a.g;
    if (!Vx || !Vy || !Vz) return jrx_fail(h, JRX_ERR_ARG, "%s: V.%s is NULL", fn, !Vx ? "Vx" : (!Vy ? "Vy" : "Vz"));
    if (!std::isfinite(dt)) return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g (must be finite)", fn, dt);
    JRX_TRY(pt_apart(h, fn, {Vx, 8 * (i64)(g.nx + 1) * (g.ny + 2) * (g.nz + 2), "V.Vx"}, S));
    JRX_TRY(pt_apart(h, fn, {Vy, 8 * (i64)(g.nx + 2) * (g.ny + 1) * (g.nz + 2), "V.Vy"}, S));
    JRX_TRY(pt_apart(h, fn, {Vz, 8 * (i64)(g.nx + 2) * (g.ny + 2) * (g.nz + 1), "V.Vz"}, S));
    JRX_TRY(jrx_check_device(h));
    a.Vx = Vx, a.Vy = Vy, a.Vz = Vz;
    a.hx = part->x0 - 0.5 * part->dx, a.hy = part->y0 - 0.5 * part->dy, a.hz = part->z0 - 0.5 * part->dz;
    a.dt = dt, a.hdt = 0.5 * dt;
    h->stat_particles_launches++;
    hipLaunchKernelGGL(k_p3_advect_rk2, p3_grid(g.nx, g.ny, g.nz), kP3Block, 0, h->stream, a);
    return op_finish(h);
}

jrx_status jrx_particles3d_move(jrx_handle *h, const jrx_particles3d *src, const jrx_particles3d *dst, const double *const *args_src, double *const *args_dst,
                                int32_t nargs, uint8_t *work, int64_t counts[5])
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "move_particles!";
    P3MoveArgs a = {};
    P3Geom d;
    PtSet S, D;
    JRX_TRY(p3_geom(h, fn, "particles (source)", src, &S, &a.src));
    JRX_TRY(p3_geom(h, fn, "particles (destination)", dst, &D, &d));
    JRX_TRY(pt_move_checks(h, fn, S, D, args_src, args_dst, nargs, work, counts));          // the byte buffer is an output too
    JRX_TRY(jrx_check_device(h));
    a.dpx = d.px, a.dpy = d.py, a.dpz = d.pz, a.dactive = d.active;
    for (int q = 0; q < nargs; q++) a.as[q] = args_src[q], a.ad[q] = args_dst[q];
    a.nargs = (int)nargs;
    a.codes = work;
    a.counts = pt_words(h);
    const dim3 grid = p3_grid(d.nx, d.ny, d.nz);
    JRX_HIP(h, hipMemsetAsync(a.counts, 0, sizeof(int64_t) * 5, h->stream));
    if (work && h->particles3d_move_codes) {
        h->stat_particles_launches += 2;
        hipLaunchKernelGGL(k_p3_move_codes, grid, kP3Block, 0, h->stream, a);
        hipLaunchKernelGGL(k_p3_move_gather, grid, kP3Block, 0, h->stream, a);
    } else {
        h->stat_particles_launches++;
        hipLaunchKernelGGL(k_p3_move, grid, kP3Block, 0, h->stream, a);
    }
    JRX_LAUNCH_CHECK(h);
    return pt_read_words(h, 0, 5, counts);
}

jrx_status jrx_particles3d_grid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles3d *part)
{
    return p3_field_op(h, "grid2particle!", k_p3_grid2particle, pF, (double *)F, part, 1, true, false);
}

jrx_status jrx_particles3d_particle2grid(jrx_handle *h, double *F, const double *pF, const jrx_particles3d *part)
{
    return p3_field_op(h, "particle2grid!", k_p3_particle2grid, (double *)pF, F, part, 1, false, false);
}

jrx_status jrx_particles3d_centroid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles3d *part)
{
    return p3_field_op(h, "centroid2particle!", k_p3_centroid2particle, pF, (double *)F, part, 0, true, true);
}

jrx_status jrx_particles3d_particle2centroid(jrx_handle *h, double *F, const double *pF, const jrx_particles3d *part)
{
    return p3_field_op(h, "particle2centroid!", k_p3_particle2centroid, (double *)pF, F, part, 0, false, false);
}

jrx_status jrx_particles3d_phase_ratios(jrx_handle *h, double *const members[8], const double *pPhases, int32_t nphase, const jrx_particles3d *part, int64_t *n_empty)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "update_phase_ratios!(particles)";
    static const char *const names[kP3Members] = {"phase_ratios.center", "phase_ratios.vertex", "phase_ratios.Vx", "phase_ratios.Vy",
                                                  "phase_ratios.Vz",     "phase_ratios.yz",     "phase_ratios.xz", "phase_ratios.xy"};
    static const int stag[kP3Members][3] = {{0, 0, 0}, {1, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};
    P3PrArgs a = {};
    PtSet S;
    JRX_TRY(p3_geom(h, fn, "particles", part, &S, &a.g));
    JRX_TRY(pt_ratio_checks(h, fn, S, members, names, stag, kP3Members, pPhases, nphase, n_empty));
    JRX_TRY(jrx_check_device(h));
    const P3Geom &g = a.g;
    for (int m = 0; m < kP3Members; m++) a.out[m] = members[m];
    a.pPhases = pPhases;
    a.n_empty = pt_words(h) + 5;
    const dim3 grid = p3_grid(g.nx + 1, g.ny + 1, g.nz + 1);
    JRX_HIP(h, hipMemsetAsync(a.n_empty, 0, sizeof(int64_t), h->stream));
    // measured at 128^3: one launch wins at nphase = 2 (1.93 against 2.50 ms), two launches at nphase = 8 (3.65 against 4.12 ms: the one-launch form holds 72
    // accumulators and runs two waves per SIMD); the counts between were not measured and take the one launch
    const bool split = h->particles3d_ratios_split == 1 || (h->particles3d_ratios_split == 2 && nphase == JRX_MAXPHASE);
    h->stat_particles_launches += split ? 2 : 1;
    dispatch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)nphase, [&](auto NN) {
        if (split) {
            // center, Vx, Vy, Vz (1 + 3 x 2 cell feeds) | vertex, yz, xz, xy (8 + 3 x 4)
            hipLaunchKernelGGL((k_p3_phase_ratios<NN(), 0x1d>), grid, kP3Block, 0, h->stream, a);
            hipLaunchKernelGGL((k_p3_phase_ratios<NN(), 0xe2>), grid, kP3Block, 0, h->stream, a);
        } else {
            hipLaunchKernelGGL((k_p3_phase_ratios<NN(), 0xff>), grid, kP3Block, 0, h->stream, a);
        }
    });
    JRX_LAUNCH_CHECK(h);
    return pt_read_words(h, 5, 1, n_empty);
}

}  // extern "C"
