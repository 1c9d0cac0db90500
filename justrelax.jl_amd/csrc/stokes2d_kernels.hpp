// stokes2d_kernels.hpp -- device-side pieces of the 2D Stokes PT iteration that both 2D drivers need: the visco-elastic path (stokes2d.hip)
// and the visco-elasto-plastic / non-linear drivers (stokes2d_vep.hip).  See stokes2d.hip for the reference citations.
#pragma once
#include "jrx_internal.hpp"

namespace {

// inverse spacings of a non-uniform Geometry (src/grid/Cartesian.jl:77-100): device arrays, all NULL on a uniform grid (then the scalars _dx, _dy apply).
// vx, vy = _di.vertex (nx | ny entries: cell sizes), cx, cy = _di.center (nx-1 | ny-1: distances of the cell centres), vxy = _di.velocity[1][2] (y spacing of the
// Vx grid with its ghost rows, ny+1), vyx = _di.velocity[2][1] (x spacing of the Vy grid, nx+1).  Which one a stencil takes is the reference's choice, kernel by
// kernel (VelocityKernels.jl:3-44,108-180,246-307, stress_rotation_particles.jl:17-29).
struct Sp2 { const double *vx, *vy, *cx, *cy, *vxy, *vyx; };
__device__ __forceinline__ double spc(const double *a, const int i, const double u) { return a ? a[i] : u; }

struct Args2 {
    jrx_stokes2d_fields f;
    const double *etatau;
    Sp2 sp;
    double _dx, _dy, dt, r, theta_dtau, eta_dtau;
    int nx, ny;
    unsigned fs, ns;      // free_slip / no_slip face masks for the velocity kernel's fused ghost update (BCF)
    double fs_dt = 0.0;   // dt * free_surface of the free-surface forms of compute_V! / compute_Res! (VelocityKernels.jl:134-180,271-307)
};

inline Args2 make_args2(const jrx_stokes2d_fields *f, const double *etatau, const jrx_stokes2d_params *p)
{
    Args2 a;
    a.f = *f; a.etatau = etatau;
    a._dx = p->_dx; a._dy = p->_dy; a.dt = p->dt; a.r = p->r; a.theta_dtau = p->theta_dtau; a.eta_dtau = p->eta_dtau;
    a.nx = (int)p->nx; a.ny = (int)p->ny;
    a.fs = p->free_slip; a.ns = p->no_slip;
    a.sp = Sp2{p->inv_spacing[0], p->inv_spacing[1], p->inv_spacing[2], p->inv_spacing[3], p->inv_spacing[4], p->inv_spacing[5]};
    return a;
}

// Blocks are dealt round-robin to the 8 XCDs, each with its own L2: block L of a 1D launch takes position (L % 8) * (T / 8) + L / 8 of the flattened
// (x fastest) node sequence, so that every XCD works on a contiguous band of rows and finds the rows j +- 1 of its stencils in its own L2
// (shear band 1024^2: k_vep_stress2d fetched 37.8 array passes from HBM for 19 needed, profiles/r02_bench2d_xcd_slabs.txt)
__device__ __forceinline__ unsigned xcd_slab_block()
{
    const unsigned L = blockIdx.x, per = gridDim.x / 8u;
    return L < per * 8u ? (L & 7u) * per + (L >> 3) : L;
}

#define CC(i_, j_) ((i_) + (i64)nx * (j_))
// compute_V! (VelocityKernels.jl:108-131); RES_ONLY stores compute_Res! (:246-269) values instead.
// BCF: the thread that updates a velocity node next to a free-slip / no-slip face also refreshes that node's ghost copy
// (free_slip.jl:1-13, no_slip.jl:1-18), which is all flow_bcs! changes once it has been applied in full one time: the other ghost
// and boundary values it writes are copies of nodes compute_V! never updates.  Saves the flow_bcs! launches of the launch-bound loop.
template <bool RES_ONLY, bool BCF>
__device__ __forceinline__ void velocity2d_cell(const Args2 &a, const int i, const int j)
{
    const int nx = a.nx, ny = a.ny;
    const double edt = a.eta_dtau;
    const double *__restrict__ P = a.f.P, *__restrict__ txy = a.f.txy, *__restrict__ et = a.etatau;
#define TXY(i_, j_) txy[(i_) + (i64)(nx + 1) * (j_)]
    const i64 c = CC(i, j);
    if (i < nx - 1) {
        const double _dx = spc(a.sp.cx, i, a._dx), _dy = spc(a.sp.vy, j, a._dy);        // _dx_c, _dy_v
        const double dP = (-P[c] + P[c + 1]) * _dx, dT = (-a.f.txx[c] + a.f.txx[c + 1]) * _dx;
        const double dS = (-TXY(i + 1, j) + TXY(i + 1, j + 1)) * _dy, av = (a.f.fx[c] + a.f.fx[c + 1]) * 0.5;
        if (RES_ONLY) a.f.Rx[i + (i64)(nx - 1) * j] = dT + dS - dP - av;
        else {
            const i64 q = (i + 1) + (i64)(nx + 1) * (j + 1);
            const double v = a.f.Vx[q] + (-dP + dT + dS - av) * edt / ((et[c] + et[c + 1]) * 0.5);
            a.f.Vx[q] = v;
            if (BCF) {      // Vx ghost rows j = 0 (bot) and j = ny+1 (top)
                if (j == 0) { if (a.fs & JRX_FACE_BOT) a.f.Vx[q - (nx + 1)] = v; else if (a.ns & JRX_FACE_BOT) a.f.Vx[q - (nx + 1)] = -v; }
                if (j == ny - 1) { if (a.fs & JRX_FACE_TOP) a.f.Vx[q + (nx + 1)] = v; else if (a.ns & JRX_FACE_TOP) a.f.Vx[q + (nx + 1)] = -v; }
            }
        }
    }
    if (j < ny - 1) {
        const double _dx = spc(a.sp.vx, i, a._dx), _dy = spc(a.sp.cy, j, a._dy);        // _dx_v, _dy_c
        const double dP = (-P[c] + P[c + nx]) * _dy, dT = (-a.f.tyy[c] + a.f.tyy[c + nx]) * _dy;
        const double dS = (-TXY(i, j + 1) + TXY(i + 1, j + 1)) * _dx, av = (a.f.fy[c] + a.f.fy[c + nx]) * 0.5;
        double corr = 0.0;
        const bool fsurf = a.fs_dt != 0.0;
        if (fsurf) {      // ρg_correction = Vy ∂(ρg_y)/∂y θ dt with θ = 1, j_N = min(j + 1, ny)
            const int jN = min(j + 1, ny - 1);
            const double drg = (a.f.fy[i + (i64)nx * jN] - a.f.fy[c]) * _dy;
            const double vy0 = a.f.Vy[(i + 1) + (i64)(nx + 2) * (j + 1)];
            corr = RES_ONLY ? (vy0 * drg) * 1.0 * a.fs_dt : vy0 * drg * 1.0 * a.fs_dt;
        }
        if (RES_ONLY) a.f.Ry[c] = fsurf ? dT + dS - dP - av + corr : dT + dS - dP - av;
        else {
            const i64 q = (i + 1) + (i64)(nx + 2) * (j + 1);
            const double rhs = fsurf ? -dP + dT + dS - av + corr : -dP + dT + dS - av;
            const double v = a.f.Vy[q] + rhs * edt / ((et[c] + et[c + nx]) * 0.5);
            a.f.Vy[q] = v;
            if (BCF) {      // Vy ghost columns i = 0 (left) and i = nx+1 (right)
                if (i == 0) { if (a.fs & JRX_FACE_LEFT) a.f.Vy[q - 1] = v; else if (a.ns & JRX_FACE_LEFT) a.f.Vy[q - 1] = -v; }
                if (i == nx - 1) { if (a.fs & JRX_FACE_RIGHT) a.f.Vy[q + 1] = v; else if (a.ns & JRX_FACE_RIGHT) a.f.Vy[q + 1] = -v; }
            }
        }
    }
#undef TXY
}

template <bool RES_ONLY, bool BCF = false>
__global__ __launch_bounds__(256) void k_velocity2d(const Args2 a)
{
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / a.nx, i = t - j * a.nx;
    if (j >= a.ny) return;
    velocity2d_cell<RES_ONLY, BCF>(a, i, j);
}
#undef CC

}   // namespace
