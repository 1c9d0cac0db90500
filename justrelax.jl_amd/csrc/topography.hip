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
//
// 3D (the second half of the file; tests/_topography3d.py is the same text in NumPy): the surface h(x, y) at the (nx + 1, ny + 1) vertex positions, linear on the
// four triangles corner-corner-centre of every cell.  k_rock_fraction3d: ONE launch, a thread per node (i, j) and per chunk of vertex rows k (64 x 4 nodes, 4 rows
// by measurement) writes the eight members that node owns; its only loads are the nine heights around (i, j); rows the surface does not cross are 1 or 0 by the
// shortcuts of the definition without evaluating a triangle.  k_advect_topography3d: a thread per vertex.  k_phases_topography3d<N>: a thread per column (i, j)
// marches k by the 2D rule.
#include "op_args.hpp"

namespace {

constexpr int kTpTX = 64, kTpTY = 4;                  // tile of nodes of k_rock_fraction2d
constexpr int kTpCols = 64;                           // columns per block of the 1D kernels
constexpr int kTpRows3 = 4;                           // vertex rows a thread of k_rock_fraction3d marches (tuning "rock_fraction3d_rows"; measured, profiles/topography3d_bench.txt)

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

// ------------------------------------------------------------------------------------------------ 3D: the surface h(x, y) at the (nx + 1, ny + 1) vertex positions
// Every cell is split into the four triangles corner-corner-centre (include/jrx.h); a quadrant is the quarter of a cell at one of its corners, two half-triangles
// of area 1/8 with the vertex values (A, mx, c) and (A, my, c).

// Ψ(a, b, c): the mean of max(g, 0) over a triangle, g linear with the sorted vertex values a <= b <= c
__device__ __forceinline__ double tp_psi(double a, double b, double c)
{
    if (c <= 0.0) return 0.0;
    if (a >= 0.0) return ((a + b) + c) / 3.0;
    if (b <= 0.0) return ((c * c) * c) / ((3.0 * (c - a)) * (c - b));
    const double na = -a;
    return ((a + b) + c) / 3.0 + ((na * na) * na) / ((3.0 * (b - a)) * (c - a));
}

// T(g1, g2, g3, H): the mean over a triangle of clamp(g, 0, H)
__device__ __forceinline__ double tp_tri(double g1, double g2, double g3, double H)
{
    const bool w1 = g2 < g1;
    const double lo = w1 ? g2 : g1, hi = w1 ? g1 : g2;
    const bool w2 = g3 < hi;
    const double c = w2 ? hi : g3, m = w2 ? g3 : hi;
    const bool w3 = m < lo;
    const double a = w3 ? m : lo, b = w3 ? lo : m;
    if (a >= H) return H;
    if (c <= 0.0) return 0.0;
    return tp_psi(a, b, c) - tp_psi(a - H, b - H, c - H);
}

// the volume of the quadrant at the corner A (X, Y: the cell's neighbouring corners along x and y, c: its centre value) inside the z range [b, b + H]
__device__ __forceinline__ double tp_quad(double A, double X, double Y, double c, double b, double H)
{
    const double mx = 0.5 * (A + X), my = 0.5 * (A + Y), ga = A - b, gc = c - b;
    return 0.125 * tp_tri(ga, mx - b, gc, H) + 0.125 * tp_tri(ga, my - b, gc, H);
}

__device__ __forceinline__ double tp_centre4(double s00, double s10, double s01, double s11) { return 0.25 * ((s00 + s10) + (s01 + s11)); }

// center[i, j, k] from the four corners of cell (i, j) and its centre value; lo, hi: the smallest and the largest corner.  Midpoints and centre lie between the
// corners and x - b is monotone in x, so lo - b >= 1 (hi - b <= 0) says that every triangle takes its first (second) shortcut: the sum is then exactly 1 (0)
__device__ __forceinline__ double tp_center3(double s00, double s10, double s01, double s11, double c, double lo, double hi, double b)
{
    if (lo - b >= 1.0) return 1.0;
    if (hi - b <= 0.0) return 0.0;
    double v = 0.0;
    v = v + tp_quad(s00, s10, s01, c, b, 1.0);
    v = v + tp_quad(s10, s00, s11, c, b, 1.0);
    v = v + tp_quad(s01, s11, s00, c, b, 1.0);
    v = v + tp_quad(s11, s01, s10, c, b, 1.0);
    return tp_clamp(v, 0.0, 1.0);
}

__device__ __forceinline__ double tp_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double tp_max(double a, double b) { return b > a ? b : a; }

struct Rf3Args {
    const double *h;
    double *center, *vertex, *Vx, *Vy, *Vz, *yz, *xz, *xy;
    double z0, idz;
    int nx, ny, nz, nbx, nby, rows;      // rows: vertex rows k a thread marches
};

// A thread per node (i, j) of the (nx + 1, ny + 1) vertex positions and per chunk of `rows` vertex rows k writes the eight members that node owns: the cell
// row k (center, Vx, Vy, xy) and the vertex row k (Vz, xz, yz, vertex).  The nine heights around (i, j) are its only loads.  A row whose z range lies below the
// smallest (above the largest) of them is all 1 (0) by the shortcuts of T, to the bit; only the rows the surface crosses evaluate the nine quadrants.
__global__ __launch_bounds__(256) void k_rock_fraction3d(const Rf3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    int blk = (int)blockIdx.x;
    const int bx = blk % a.nbx;
    blk /= a.nbx;
    const int by = blk % a.nby, bz = blk / a.nby;
    const int i = bx * kTpTX + (int)threadIdx.x, j = by * kTpTY + (int)threadIdx.y;
    if (i > nx || j > ny) return;
    const bool hasl = i > 0, hasr = i < nx, hasd = j > 0, hasu = j < ny;
    const int im = hasl ? i - 1 : i, ip = hasr ? i + 1 : i, jm = hasd ? j - 1 : j, jp = hasu ? j + 1 : j, sx = nx + 1;      // a missing neighbour: the node itself (unused)
    const double z0 = a.z0, idz = a.idz;
    const double smm = (a.h[jm * sx + im] - z0) * idz, s0m = (a.h[jm * sx + i] - z0) * idz, spm = (a.h[jm * sx + ip] - z0) * idz;
    const double sm0 = (a.h[j * sx + im] - z0) * idz, s00 = (a.h[j * sx + i] - z0) * idz, sp0 = (a.h[j * sx + ip] - z0) * idz;
    const double smp = (a.h[jp * sx + im] - z0) * idz, s0p = (a.h[jp * sx + i] - z0) * idz, spp = (a.h[jp * sx + ip] - z0) * idz;
    const double cmm = tp_centre4(smm, s0m, sm0, s00), cpm = tp_centre4(s0m, spm, s00, sp0), cmp = tp_centre4(sm0, s00, smp, s0p), cpp = tp_centre4(s00, sp0, s0p, spp);
    const double lo = tp_min(tp_min(tp_min(tp_min(smm, s0m), tp_min(spm, sm0)), tp_min(tp_min(s00, sp0), tp_min(smp, s0p))), spp);
    const double hi = tp_max(tp_max(tp_max(tp_max(smm, s0m), tp_max(spm, sm0)), tp_max(tp_max(s00, sp0), tp_max(smp, s0p))), spp);
    const double Wx = hasl && hasr ? 1.0 : 0.5, Wy = hasd && hasu ? 1.0 : 0.5;
    const double Wv = 0.25 * (double)((int)(hasl && hasd) + (int)(hasr && hasd) + (int)(hasl && hasu) + (int)(hasr && hasu));
    const int k0 = bz * a.rows, k1 = k0 + a.rows < nz + 1 ? k0 + a.rows : nz + 1;
    for (int k = k0; k < k1; k++) {
#pragma unroll 1
        for (int r = k < nz ? 0 : 1; r < 2; r++) {      // r = 0: the cell row k, r = 1: the vertex row k
            const double kd = (double)k;
            const double bv = kd - 0.5 > 0.0 ? kd - 0.5 : 0.0, tv = kd + 0.5 < (double)nz ? kd + 0.5 : (double)nz;
            const double b = r ? bv : kd, H = r ? tv - bv : 1.0;
            double vc, vx, vy, vv;
            if (lo - b >= H) vc = vx = vy = vv = 1.0;
            else if (hi - b <= 0.0) vc = vx = vy = vv = 0.0;
            else {
                const double q1 = tp_quad(s00, sp0, s0p, cpp, b, H), q2 = tp_quad(sp0, s00, spp, cpp, b, H), q3 = tp_quad(s0p, spp, s00, cpp, b, H);
                const double q4 = tp_quad(spp, s0p, sp0, cpp, b, H), q5 = tp_quad(s00, sm0, s0p, cmp, b, H), q6 = tp_quad(s0p, smp, s00, cmp, b, H);
                const double q7 = tp_quad(s00, sp0, s0m, cpm, b, H), q8 = tp_quad(sp0, s00, spm, cpm, b, H), q9 = tp_quad(s00, sm0, s0m, cmm, b, H);
                double t = 0.0;
                t = t + q1, t = t + q2, t = t + q3, t = t + q4;
                vc = tp_clamp(t / (1.0 * H), 0.0, 1.0);
                t = 0.0;
                if (hasl) t = t + q5, t = t + q6;
                if (hasr) t = t + q1, t = t + q3;
                vx = tp_clamp(t / (Wx * H), 0.0, 1.0);
                t = 0.0;
                if (hasd) t = t + q7, t = t + q8;
                if (hasu) t = t + q1, t = t + q2;
                vy = tp_clamp(t / (Wy * H), 0.0, 1.0);
                t = 0.0;
                if (hasl && hasd) t = t + q9;
                if (hasr && hasd) t = t + q7;
                if (hasl && hasu) t = t + q5;
                if (hasr && hasu) t = t + q1;
                vv = tp_clamp(t / (Wv * H), 0.0, 1.0);
            }
            double *const pc = r ? a.Vz : a.center, *const px = r ? a.xz : a.Vx, *const py = r ? a.yz : a.Vy, *const pv = r ? a.vertex : a.xy;
            if (hasr && hasu) pc[(k * ny + j) * nx + i] = vc;
            if (hasu) px[(k * ny + j) * (nx + 1) + i] = vx;
            if (hasr) py[(k * (ny + 1) + j) * nx + i] = vy;
            pv[(k * (ny + 1) + j) * (nx + 1) + i] = vv;
        }
    }
}

struct Adv3Args {
    double *h;
    const double *h_old, *Vx, *Vy, *Vz;      // Vx (nx + 1, ny + 2, nz + 2), Vy (nx + 2, ny + 1, nz + 2), Vz (nx + 2, ny + 2, nz + 1)
    double z0, idx, idy, idz, dt;
    int nx, ny, nz, nbx;
};

__global__ __launch_bounds__(256) void k_advect_topography3d(const Adv3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const int i = ((int)blockIdx.x % a.nbx) * kTpTX + (int)threadIdx.x, j = ((int)blockIdx.x / a.nbx) * kTpTY + (int)threadIdx.y;
    if (i > nx || j > ny) return;
    const int sx = nx + 1;
    const double sig = tp_clamp((a.h_old[j * sx + i] - a.z0) * a.idz, 0.0, (double)nz);
    int k0 = (int)floor(sig);
    k0 = k0 < nz - 1 ? k0 : nz - 1;
    const double t = sig - (double)k0;
    double v[3][2];
#pragma unroll
    for (int l = 0; l < 2; l++) {
        const int k = k0 + l;
        const double *px = a.Vx + (k * (ny + 2) + j) * (nx + 1) + i, *py = a.Vy + (k * (ny + 1) + j) * (nx + 2) + i, *pz = a.Vz + (k * (ny + 2) + j) * (nx + 2) + i;
        const int px_k = (ny + 2) * (nx + 1), py_k = (ny + 1) * (nx + 2);
        v[0][l] = 0.25 * ((px[0] + px[px_k]) + (px[nx + 1] + px[nx + 1 + px_k]));          // vxv(i, j, k): Vx[i, j .. j + 1, k .. k + 1]
        v[1][l] = 0.25 * ((py[0] + py[py_k]) + (py[1] + py[1 + py_k]));                    // vyv(i, j, k): Vy[i .. i + 1, j, k .. k + 1]
        v[2][l] = 0.25 * ((pz[0] + pz[1]) + (pz[nx + 2] + pz[nx + 3]));                    // vzv(i, j, k): Vz[i .. i + 1, j .. j + 1, k]
    }
    const double vx = (1.0 - t) * v[0][0] + t * v[0][1], vy = (1.0 - t) * v[1][0] + t * v[1][1], vz = (1.0 - t) * v[2][0] + t * v[2][1];
    const double xi = tp_clamp((double)i - (vx * a.dt) * a.idx, 0.0, (double)nx), eta = tp_clamp((double)j - (vy * a.dt) * a.idy, 0.0, (double)ny);
    int i0 = (int)floor(xi), j0 = (int)floor(eta);
    i0 = i0 < nx - 1 ? i0 : nx - 1;
    j0 = j0 < ny - 1 ? j0 : ny - 1;
    const double r = xi - (double)i0, q = eta - (double)j0;
    const double *ho = a.h_old + j0 * sx + i0;
    const double lo = (1.0 - r) * ho[0] + r * ho[1], hi = (1.0 - r) * ho[sx] + r * ho[sx + 1];
    a.h[j * sx + i] = ((1.0 - q) * lo + q * hi) + vz * a.dt;
}

struct Ph3Args {
    double *c[JRX_MAXPHASE];
    const double *h;
    double z0, idz;
    int nx, ny, nz, nbx, air;      // air: 0-based
};

template <int N>
__global__ __launch_bounds__(256) void k_phases_topography3d(const Ph3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz, air = a.air;
    const int i = ((int)blockIdx.x % a.nbx) * kTpTX + (int)threadIdx.x, j = ((int)blockIdx.x / a.nbx) * kTpTY + (int)threadIdx.y;
    if (i >= nx || j >= ny) return;
    const double *hp = a.h + j * (nx + 1) + i;
    const double s00 = (hp[0] - a.z0) * a.idz, s10 = (hp[1] - a.z0) * a.idz, s01 = (hp[nx + 1] - a.z0) * a.idz, s11 = (hp[nx + 2] - a.z0) * a.idz;
    const double cc = tp_centre4(s00, s10, s01, s11);
    const double lo = tp_min(tp_min(s00, s10), tp_min(s01, s11)), hi = tp_max(tp_max(s00, s10), tp_max(s01, s11));
    const int first = air == 0 ? 1 : 0;                               // the lowest non-air index (N == 1: none, and no rock field is touched)
    double p[N], c[N];
#pragma unroll
    for (int k = 0; k < N; k++) p[k] = k == first ? 1.0 : 0.0;
#pragma unroll 1
    for (int kz = 0; kz < nz; kz++) {
        const int lin = (kz * ny + j) * nx + i;
        const double f = tp_center3(s00, s10, s01, s11, cc, lo, hi, (double)kz);
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

// ------------------------------------------------------------------------------------------------ host: one body per operator, ND = 2 or 3
// extents >= 1 and every array (the largest is the ni .+ 2 box of the velocities) below 2^31 entries
jrx_status tp_extents(jrx_handle *h, const char *fn, const int64_t *n, int ND)
{
    if (!op_extents_ok(n, ND)) return jrx_fail(h, JRX_ERR_ARG, "%s: extents %s (each must be >= 1)", fn, op_list(n, ND, " x ").s);
    if (op_2g(op_count(n, ND, 2))) return jrx_fail(h, JRX_ERR_ARG, "%s: the ni .+ 2 box has 2^31 or more entries (32-bit offsets)", fn);
    return JRX_OK;
}

// compute_rock_fraction!: the members of ϕ in the order of the 3D entry point, of which 2D has the first four; u0, _du: origin and inverse spacing of the
// vertical axis (y in 2D, z in 3D)
jrx_status tp_rock_fraction(jrx_handle *h, int ND, double *const *out, const double *topo_h, const int64_t n[3], double u0, double _du)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "compute_rock_fraction!";
    static const char *const names[8] = {"ϕ.center", "ϕ.vertex", "ϕ.Vx", "ϕ.Vy", "ϕ.Vz", "ϕ.yz", "ϕ.xz", "ϕ.xy"};
    static const int stag[8][3] = {{0, 0, 0}, {1, 1, 1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};
    const int NM = ND == 2 ? 4 : 8, ax = "xyz"[ND - 1];
    OpArr o[8], in[1] = {{topo_h, 0, "topo.h"}};
    for (int m = 0; m < NM; m++) o[m] = OpArr{out[m], 0, names[m]};
    JRX_TRY(op_present(h, fn, o, NM));
    JRX_TRY(op_present(h, fn, in, 1));
    JRX_TRY(tp_extents(h, fn, n, ND));
    if (!op_finite({u0, _du})) return jrx_fail(h, JRX_ERR_ARG, "%s: %c0 = %g, _d%c = %g (both must be finite)", fn, ax, u0, ax, _du);
    for (int m = 0; m < NM; m++) o[m].bytes = op_bytes(n, ND, stag[m][0], stag[m][1], stag[m][2]);
    in[0].bytes = op_bytes(n, ND - 1, 1, 1);          // the height field: a value per vertex of the ND - 1 horizontal axes
    if (const OpClash c = op_disjoint(o, NM, in, 1))
        return c.two ? jrx_fail(h, JRX_ERR_ARG, "%s: outputs %s and %s overlap", fn, o[c.a].name, o[c.b].name)
                     : jrx_fail(h, JRX_ERR_ARG, "%s: output %s overlaps topo.h", fn, o[c.a].name);
    JRX_TRY(jrx_check_device(h));
    const int64_t nx = n[0], ny = n[1], nz = n[2];
    h->stat_rock_fraction_calls++;
    if (ND == 2) {
        RfArgs a = {topo_h, out[0], out[1], out[2], out[3], u0, _du, (int)nx, (int)ny, (int)((nx + 1 + kTpTX - 1) / kTpTX)};
        const int64_t nb = (int64_t)a.nbx * ((ny + 1 + kTpTY - 1) / kTpTY);      // below 2^31: the box is
        hipLaunchKernelGGL(k_rock_fraction2d, dim3((unsigned)nb), dim3(kTpTX, kTpTY), 0, h->stream, a);
        return op_finish(h);
    }
    int rows = h->rock_fraction3d_rows > 0 ? h->rock_fraction3d_rows : kTpRows3;
    if (rows > nz + 1) rows = (int)(nz + 1);      // a deeper march is the whole column; keeps k0 + rows inside an int
    Rf3Args a = {topo_h, out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], u0, _du, (int)nx, (int)ny, (int)nz, (int)((nx + 1 + kTpTX - 1) / kTpTX),
                 (int)((ny + 1 + kTpTY - 1) / kTpTY), rows};
    const int64_t nb = (int64_t)a.nbx * a.nby * ((nz + 1 + rows - 1) / rows);      // below 2^31: no more blocks than nodes of the ni .+ 1 box
    hipLaunchKernelGGL(k_rock_fraction3d, dim3((unsigned)nb), dim3(kTpTX, kTpTY), 0, h->stream, a);
    return op_finish(h);
}

// advect_topography!: V the ND velocity components with their ghost layers, _di the ND inverse spacings
jrx_status tp_advect(jrx_handle *h, int ND, double *topo_h, double *topo_h_old, const double *const *V, const int64_t n[3], double u0, const double *_di, double dt)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "advect_topography!";
    static const char *const vnames[3] = {"V.Vx", "V.Vy", "V.Vz"};
    OpArr o[2] = {{topo_h, 0, "topo.h"}, {topo_h_old, 0, "topo.h_old"}}, in[3];
    for (int c = 0; c < ND; c++) in[c] = OpArr{V[c], 0, vnames[c]};
    JRX_TRY(op_present(h, fn, o, 2));
    JRX_TRY(op_present(h, fn, in, ND));
    JRX_TRY(tp_extents(h, fn, n, ND));
    if (ND == 2 && !op_finite({dt, _di[0], _di[1], u0}))
        return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g, _dx = %g, _dy = %g, y0 = %g (all must be finite)", fn, dt, _di[0], _di[1], u0);
    if (ND == 3 && !op_finite({dt, _di[0], _di[1], _di[2], u0}))
        return jrx_fail(h, JRX_ERR_ARG, "%s: dt = %g, _dx = %g, _dy = %g, _dz = %g, z0 = %g (all must be finite)", fn, dt, _di[0], _di[1], _di[2], u0);
    const i64 nh = op_bytes(n, ND - 1, 1, 1);          // bytes of a height field
    o[0].bytes = o[1].bytes = nh;
    for (int c = 0; c < ND; c++) in[c].bytes = op_vel_bytes(n, ND, c);
    if (const OpClash c = op_disjoint(o, 2, in, ND)) return jrx_fail(h, JRX_ERR_ARG, "%s: output %s overlaps %s", fn, o[c.a].name, (c.two ? o : in)[c.b].name);
    JRX_TRY(jrx_check_device(h));
    const int64_t nx = n[0], ny = n[1], nz = n[2];
    h->stat_topography_advect_calls++;
    JRX_HIP(h, hipMemcpyAsync(topo_h_old, topo_h, (size_t)nh, hipMemcpyDeviceToDevice, h->stream));
    if (ND == 2) {
        AdvArgs a = {topo_h, topo_h_old, V[0], V[1], u0, _di[0], _di[1], dt, (int)nx, (int)ny};
        hipLaunchKernelGGL(k_advect_topography2d, dim3((unsigned)((nx + 1 + kTpCols - 1) / kTpCols)), dim3(kTpCols), 0, h->stream, a);
    } else {
        Adv3Args a = {topo_h, topo_h_old, V[0], V[1], V[2], u0, _di[0], _di[1], _di[2], dt, (int)nx, (int)ny, (int)nz, (int)((nx + 1 + kTpTX - 1) / kTpTX)};
        hipLaunchKernelGGL(k_advect_topography3d, dim3((unsigned)((int64_t)a.nbx * ((ny + 1 + kTpTY - 1) / kTpTY))), dim3(kTpTX, kTpTY), 0, h->stream, a);
    }
    return op_finish(h);
}

// update_phases_given_topography!
jrx_status tp_phases(jrx_handle *h, int ND, double *const *phases, int32_t nphase, const double *topo_h, const int64_t n[3], double u0, double _du, int32_t air_phase)
{
    if (!h) return JRX_ERR_ARG;
    const char *fn = "update_phases_given_topography!";
    const int ax = "xyz"[ND - 1];
    if (!phases) return jrx_fail(h, JRX_ERR_ARG, "%s: phases is NULL", fn);
    if (nphase < 1 || nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phase fields (1 .. %d are built)", fn, (int)nphase, JRX_MAXPHASE);
    if (air_phase < 1 || air_phase > nphase) return jrx_fail(h, JRX_ERR_ARG, "%s: air_phase %d outside 1 .. %d", fn, (int)air_phase, (int)nphase);
    for (int k = 0; k < nphase; k++)
        if (!phases[k]) return jrx_fail(h, JRX_ERR_ARG, "%s: phase field %d is NULL", fn, k + 1);
    if (!topo_h) return jrx_fail(h, JRX_ERR_ARG, "%s: topo.h is NULL", fn);
    JRX_TRY(tp_extents(h, fn, n, ND));
    if (!op_finite({u0, _du})) return jrx_fail(h, JRX_ERR_ARG, "%s: %c0 = %g, _d%c = %g (both must be finite)", fn, ax, u0, ax, _du);
    OpArr o[JRX_MAXPHASE];
    for (int k = 0; k < nphase; k++) o[k] = OpArr{phases[k], op_bytes(n, ND, 0, 0, 0), nullptr};
    const OpArr in[1] = {{topo_h, op_bytes(n, ND - 1, 1, 1), nullptr}};
    if (const OpClash c = op_disjoint(o, nphase, in, 1))
        return c.two ? jrx_fail(h, JRX_ERR_ARG, "%s: phase fields %d and %d overlap", fn, c.a + 1, c.b + 1)
                     : jrx_fail(h, JRX_ERR_ARG, "%s: phase field %d overlaps topo.h", fn, c.a + 1);
    JRX_TRY(jrx_check_device(h));
    const int64_t nx = n[0], ny = n[1], nz = n[2];
    h->stat_topography_phase_calls++;
    if (ND == 2) {
        PhArgs a = {};
        for (int k = 0; k < nphase; k++) a.c[k] = phases[k];
        a.h = topo_h, a.y0 = u0, a.idy = _du, a.nx = (int)nx, a.ny = (int)ny, a.air = (int)air_phase - 1;
        dispatch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)nphase, [&](auto NN) {
            hipLaunchKernelGGL((k_phases_topography2d<NN()>), dim3((unsigned)((nx + kTpCols - 1) / kTpCols)), dim3(kTpCols), 0, h->stream, a);
        });
        return op_finish(h);
    }
    Ph3Args a = {};
    for (int k = 0; k < nphase; k++) a.c[k] = phases[k];
    a.h = topo_h, a.z0 = u0, a.idz = _du, a.nx = (int)nx, a.ny = (int)ny, a.nz = (int)nz, a.nbx = (int)((nx + kTpTX - 1) / kTpTX), a.air = (int)air_phase - 1;
    const unsigned nb = (unsigned)((int64_t)a.nbx * ((ny + kTpTY - 1) / kTpTY));
    dispatch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)nphase, [&](auto NN) {
        hipLaunchKernelGGL((k_phases_topography3d<NN()>), dim3(nb), dim3(kTpTX, kTpTY), 0, h->stream, a);
    });
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_compute_rock_fraction2d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *topo_h, int64_t nx, int64_t ny, double y0,
                                       double _dy)
{
    double *const out[4] = {center, vertex, Vx, Vy};
    const int64_t n[3] = {nx, ny, 1};
    return tp_rock_fraction(h, 2, out, topo_h, n, y0, _dy);
}

jrx_status jrx_compute_rock_fraction3d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, double *Vz, double *yz, double *xz, double *xy,
                                       const double *topo_h, int64_t nx, int64_t ny, int64_t nz, double z0, double _dz)
{
    double *const out[8] = {center, vertex, Vx, Vy, Vz, yz, xz, xy};
    const int64_t n[3] = {nx, ny, nz};
    return tp_rock_fraction(h, 3, out, topo_h, n, z0, _dz);
}

jrx_status jrx_advect_topography2d(jrx_handle *h, double *topo_h, double *topo_h_old, const double *Vx, const double *Vy, int64_t nx, int64_t ny, double y0,
                                   double _dx, double _dy, double dt)
{
    const double *const V[2] = {Vx, Vy};
    const int64_t n[3] = {nx, ny, 1};
    const double _di[2] = {_dx, _dy};
    return tp_advect(h, 2, topo_h, topo_h_old, V, n, y0, _di, dt);
}

jrx_status jrx_advect_topography3d(jrx_handle *h, double *topo_h, double *topo_h_old, const double *Vx, const double *Vy, const double *Vz, int64_t nx, int64_t ny,
                                   int64_t nz, double z0, double _dx, double _dy, double _dz, double dt)
{
    const double *const V[3] = {Vx, Vy, Vz};
    const int64_t n[3] = {nx, ny, nz};
    const double _di[3] = {_dx, _dy, _dz};
    return tp_advect(h, 3, topo_h, topo_h_old, V, n, z0, _di, dt);
}

jrx_status jrx_update_phases_topography2d(jrx_handle *h, double *const *phases, int32_t nphase, const double *topo_h, int64_t nx, int64_t ny, double y0, double _dy,
                                          int32_t air_phase)
{
    const int64_t n[3] = {nx, ny, 1};
    return tp_phases(h, 2, phases, nphase, topo_h, n, y0, _dy, air_phase);
}

jrx_status jrx_update_phases_topography3d(jrx_handle *h, double *const *phases, int32_t nphase, const double *topo_h, int64_t nx, int64_t ny, int64_t nz, double z0,
                                          double _dz, int32_t air_phase)
{
    const int64_t n[3] = {nx, ny, nz};
    return tp_phases(h, 3, phases, nphase, topo_h, n, z0, _dz, air_phase);
}

}  // extern "C"
