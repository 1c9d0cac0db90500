// stokes3d_vs.hip -- 3D variational Stokes (free surface through a rock-ratio mask ϕ) for gfx950: masked kernels and driver.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/variational_stokes/Stokes3D.jl:14-238 (_solve_VS!), mask.jl:180-186,220-269,324-392 (isvalid_c,
// isvalid_vx / _vy / _vz, isvalid_yz / _xz / _xy), VelocityKernels.jl:6-12,96-154 (compute_∇V!, compute_strain_rate! 3D), StressKernels.jl:173-508
// (update_stresses_center_vertex! 3D) with the clamped stencils of src/stokes/StressKernels.jl:604-668, rheology/Viscosity.jl:599-650 (compute_phase_viscosity,
// correct_phase_ratio); compute_P!, update_ρg!, flow_bcs!, the norms' reductions and the epilogue operators are the unmasked ones of the 3D drivers.
// The masked 3D compute_V! of the reference (VelocityKernels.jl:408-487) cannot run -- it calls averages nothing defines and its masked differences resolve to
// forms that cross two planes and read past τxy -- so k_vs3_velocity is the working masked 2D kernel (:355-399) written one dimension up, on the index triples
// of the unmasked 3D kernel (src/stokes/VelocityKernels.jl:215-238); include/jrx.h states the form.
//
// Per PT iteration, three launches as in the 2D sibling (stokes2d_vs.hip): k_vs3_pre (compute_maxloc!, masked ∇V, compute_P!, masked ε, update_ρg!,
// update_viscosity_τII!; the relaxed η goes to a second array, the window of compute_maxloc! reads the neighbours' old values) -> k_vs3_stress (the three edge
// families and the centre of a node in one thread; new edge stresses and new τxx, τyy, τzz go to second sets, adopted by pointer swap, so every update reads the
// stresses of the previous iteration where the reference's single launch races) -> k_vs3_velocity -> flow_bcs!.
// ϕ is constant during a solve: the seven validity predicates are evaluated once per call into one byte per node of the ni .+ 1 box (k_vs3_flags).
// Not built: non-uniform spacing, more than one rank, free-surface stabilisation, graph replay of unobserved iterations.
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_material.hpp"

namespace {

enum : unsigned char { VS3_C = 1, VS3_YZ = 2, VS3_XZ = 4, VS3_XY = 8, VS3_VX = 16, VS3_VY = 32, VS3_VZ = 64 };

struct Vs3Args {
    jrx_vep3d_fields f;
    jrx_rheology rh;
    jrx_rock_ratio3d phi;
    const unsigned char *flags;      // [(nx+1)(ny+1)(nz+1)]: the predicates of node (i, j, k) at index i + (nx+1) (j + (ny+1) k)
    const double *etatau, *Kc, *Gc;
    const double *eta_lin;           // linear laws: the phase viscosity of a cell, computed once per solve (nullptr: from the ratios per call)
    double *theta, *lam;
    double *lamv[3], *tnew[3];       // λv and where the edge families write the new τyz, τxz, τxy
    double *cnew[3];                 // where the centres write the new τxx, τyy, τzz (the edge families average the old ones)
    double *eta_out;                 // where the pre kernel writes the relaxed η (read from f.eta)
    double _dx, _dy, _dz, dt, r, theta_dtau, eta_dtau, rel, nu, cut_lo, cut_hi;
    int nx, ny, nz, air;
    bool soft, tg, vfields, vinv, vtau, rho;
};

#define NODE3(n1_, n2_)                                                 \
    const int t_ = blockIdx.x * blockDim.x + threadIdx.x;               \
    const int j = t_ / (n1_), i = t_ - j * (n1_), k = blockIdx.y;       \
    if (j >= (n2_)) return;
#define GRID3(n1_, n2_, n3_) dim3((unsigned)(((i64)(n1_) * (n2_) + 255) / 256), (unsigned)(n3_))
#define C3(A, i, j, k) (A)[(i) + (i64)nx * ((j) + (i64)ny * (k))]
#define EYZ(A, i, j, k) (A)[(i) + (i64)nx * ((j) + (i64)(ny + 1) * (k))]
#define EXZ(A, i, j, k) (A)[(i) + (i64)(nx + 1) * ((j) + (i64)ny * (k))]
#define EXY(A, i, j, k) (A)[(i) + (i64)(nx + 1) * ((j) + (i64)(ny + 1) * (k))]
#define N3(A, i, j, k) (A)[(i) + (i64)(nx + 1) * ((j) + (i64)(ny + 1) * (k))]
#define VX(i_, j_, k_) Vx[(i_) + (i64)(nx + 1) * ((j_) + (i64)(ny + 2) * (k_))]
#define VY(i_, j_, k_) Vy[(i_) + (i64)(nx + 2) * ((j_) + (i64)(ny + 1) * (k_))]
#define VZ(i_, j_, k_) Vz[(i_) + (i64)(nx + 2) * ((j_) + (i64)(ny + 2) * (k_))]

// isvalid_c, isvalid_yz / _xz / _xy, isvalid_vx / _vy / _vz (mask.jl:180-186,220-269,324-392), 0-based.  ϕ.Vx is (nx+1, ny, nz), ϕ.Vy (nx, ny+1, nz), ϕ.Vz
// (nx, ny, nz+1), ϕ.vertex ni .+ 1: no ghost nodes.  The shear predicates read the vertices at the two ends of the edge and the four velocity nodes around it
// (clamped to their arrays); ϕ.yz / ϕ.xz / ϕ.xy enter the momentum kernel only
__global__ __launch_bounds__(256) void k_vs3_flags(unsigned char *__restrict__ flags, const jrx_rock_ratio3d phi, int nx, int ny, int nz)
{
    NODE3(nx + 1, ny + 1)
#define PVX(i_, j_, k_) (phi.Vx[(i_) + (i64)(nx + 1) * ((j_) + (i64)ny * (k_))] > 0)
#define PVY(i_, j_, k_) (phi.Vy[(i_) + (i64)nx * ((j_) + (i64)(ny + 1) * (k_))] > 0)
#define PVZ(i_, j_, k_) (phi.Vz[(i_) + (i64)nx * ((j_) + (i64)ny * (k_))] > 0)
#define PVT(i_, j_, k_) (N3(phi.vertex, i_, j_, k_) > 0)
    const int il = max(i - 1, 0), ir = min(i, nx - 1), jl = max(j - 1, 0), jr = min(j, ny - 1), kl = max(k - 1, 0), kr = min(k, nz - 1);
    unsigned char fl = 0;
    if (i < nx && j < ny && k < nz && PVX(i, j, k) && PVX(i + 1, j, k) && PVY(i, j, k) && PVY(i, j + 1, k) && PVZ(i, j, k) && PVZ(i, j, k + 1) &&
        C3(phi.center, i, j, k) > 0)
        fl |= VS3_C;
    if (i < nx && PVT(i, j, k) && PVT(i + 1, j, k) && PVZ(i, jl, k) && PVZ(i, jr, k) && PVY(i, j, kl) && PVY(i, j, kr)) fl |= VS3_YZ;
    if (j < ny && PVT(i, j, k) && PVT(i, j + 1, k) && PVZ(il, j, k) && PVZ(ir, j, k) && PVX(i, j, kl) && PVX(i, j, kr)) fl |= VS3_XZ;
    if (k < nz && PVT(i, j, k) && PVT(i, j, k + 1) && PVX(i, jl, k) && PVX(i, jr, k) && PVY(il, j, k) && PVY(ir, j, k)) fl |= VS3_XY;
    if (j < ny && k < nz && PVX(i, j, k)) fl |= VS3_VX;
    if (i < nx && k < nz && PVY(i, j, k)) fl |= VS3_VY;
    if (i < nx && j < ny && PVZ(i, j, k)) fl |= VS3_VZ;
#undef PVX
#undef PVY
#undef PVZ
#undef PVT
    N3(flags, i, j, k) = fl;
}

// compute_phase_viscosity (rheology/Viscosity.jl:599-619) of the ratios correct_phase_ratio (:638-650) leaves, as in stokes2d_vs.hip: air is 1-based, 0 = none;
// `≈ 1` is isapprox with rtol = sqrt(eps).  Zero for the air phase, r / Σ r of the others (summed in phase order) for the rest; all zero where the air ratio ≈ 1,
// whose phase average is inv(0).  Every phase's law is evaluated in a loop all lanes walk together (a return from inside it indexes the table per lane and
// puts the argument struct into scratch memory); the first phase above 0.999 wins.  air = 0: the arithmetic of mat_phase_viscosity
__device__ __forceinline__ double vs3_phase_viscosity(const jrx_rheology &rh, const double *r, const int air, double AII, double T, double P, bool tau)
{
    double s = 1.0;
    if (air > 0) {
        const double ra = r[air - 1];
        if (fabs(ra - 1.0) <= 1.4901161193847656e-08 * fmax(fabs(ra), 1.0)) return 1.0 / 0.0;
        s = 0.0;
        for (int q = 0; q < rh.nphase; q++) s += q == air - 1 ? 0.0 : r[q];
    }
    double x = 0.0, dom = 0.0;
    bool has = false;
    for (int q = 0; q < rh.nphase; q++) {
        const double c = air > 0 ? (q == air - 1 ? 0.0 : r[q] / s) : r[q];
        const double v = mat_viscosity(rh, q, AII, T, P, tau);
        if (!has && c > 0.999) { dom = v; has = true; }
        if (c != 0.0) x += (1.0 / v) * c;
    }
    return has ? dom : 1.0 / x;
}

// compute_viscosity_kernel! at a cell (rheology/Viscosity.jl:455-503): the invariant of @stress / @strain with the shear components gathered from the cell's
// twelve edges, eps() on the normal components when those vanish; T at I .+ 1 of a ghosted args.T (local_viscosity_args :513-523)
__device__ __forceinline__ double vs3_visc_cell(const Vs3Args &a, const int i, const int j, const int k)
{
    const int nx = a.nx, ny = a.ny;
    const i64 c = i + (i64)nx * (j + (i64)ny * k);
    if (a.eta_lin) return a.eta_lin[c];
    const double *r = a.f.phase_c + (i64)a.rh.nphase * c;
    if (!a.vfields) return vs3_phase_viscosity(a.rh, r, a.air, 0.0, 0.0, 0.0, a.vtau);
    double AII = 0.0;
    if (a.vinv) {
        const bool tau = a.vtau;
        const double *xx = tau ? a.f.txx : a.f.exx, *yy = tau ? a.f.tyy : a.f.eyy, *zz = tau ? a.f.tzz : a.f.ezz;
        const double *yz = tau ? a.f.tyz : a.f.eyz, *xz = tau ? a.f.txz : a.f.exz, *xy = tau ? a.f.txy : a.f.exy;
        const double a0 = (xx[c] == 0.0 && yy[c] == 0.0 && zz[c] == 0.0) ? 2.220446049250313e-16 : 0.0;
        const double x = xx[c] + a0, y = yy[c] + -a0 * 0.5, z = zz[c] + -a0 * 0.5;
        const double p0 = EYZ(yz, i, j, k), p1 = EYZ(yz, i, j + 1, k), p2 = EYZ(yz, i, j, k + 1), p3 = EYZ(yz, i, j + 1, k + 1);
        const double q0 = EXZ(xz, i, j, k), q1 = EXZ(xz, i + 1, j, k), q2 = EXZ(xz, i, j, k + 1), q3 = EXZ(xz, i + 1, j, k + 1);
        const double r0 = EXY(xy, i, j, k), r1 = EXY(xy, i + 1, j, k), r2 = EXY(xy, i, j + 1, k), r3 = EXY(xy, i + 1, j + 1, k);
        AII = sqrt(0.5 * (x * x + y * y + z * z) + 0.25 * (p0 * p0 + p1 * p1 + p2 * p2 + p3 * p3) + 0.25 * (q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3) +
                   0.25 * (r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3));
    }
    const double T = !a.f.T ? 0.0 : (a.tg ? a.f.T[(i + 1) + (i64)(nx + 2) * ((j + 1) + (i64)(ny + 2) * (k + 1))] : a.f.T[c]);
    return vs3_phase_viscosity(a.rh, r, a.air, AII, T, a.f.P[c], a.vtau);
}
// η <- clamp(ν η_phase + (1 - ν) η)
__device__ __forceinline__ void vs3_visc_at(const Vs3Args &a, const int i, const int j, const int k, double *eta_out)
{
    const i64 c = i + (i64)a.nx * (j + (i64)a.ny * k);
    const double e = vs3_visc_cell(a, i, j, k) * a.nu + a.f.eta[c] * (1.0 - a.nu);
    eta_out[c] = fmin(fmax(e, a.cut_lo), a.cut_hi);
}
__global__ __launch_bounds__(256) void k_vs3_visc(const Vs3Args a)
{
    NODE3(a.nx, a.ny)
    vs3_visc_at(a, i, j, k, a.f.eta);
}

// update_ρg! of a cell: args.T is read at the cell's own [i, j, k] of a ghosted thermal.T (BuoyancyForces.jl:52)
__device__ __forceinline__ double vs3_rhog(const Vs3Args &a, const int i, const int j, const int k)
{
    const int nx = a.nx, ny = a.ny;
    const i64 c = i + (i64)nx * (j + (i64)ny * k);
    const double T = !a.f.T ? 0.0 : (a.tg ? a.f.T[i + (i64)(nx + 2) * (j + (i64)(ny + 2) * k)] : a.f.T[c]);
    return mat_density_ratio(a.rh, a.f.phase_c + (i64)a.rh.nphase * c, T, a.f.P[c]) * a.rh.gravity;
}

// FULL: compute_maxloc!(ητ, η) of the own cell, masked compute_∇V! (VelocityKernels.jl:6-12), compute_P! (phase form, θ; ητ in the η slot), update_ρg! (a.rho),
// masked compute_strain_rate! (:96-154), update_viscosity_τII! (η from f.eta to eta_out).  !FULL: ∇V and ε alone.
// The strain-rate kernel writes NOTHING at an invalid node (it does not zero it, unlike the 2D one): the stress update's clamped averages read what the array held.
template <bool FULL>
__global__ __launch_bounds__(256) void k_vs3_pre(const Vs3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    NODE3(nx + 1, ny + 1)
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy, *__restrict__ Vz = a.f.Vz;
    const unsigned char fl = N3(a.flags, i, j, k);
    if (i < nx && j < ny && k < nz) {
        const i64 c = i + (i64)nx * (j + (i64)ny * k);
        const bool valid = (fl & VS3_C) != 0;
        const double dxi = (-VX(i, j + 1, k + 1) + VX(i + 1, j + 1, k + 1)) * a._dx;
        const double dyi = (-VY(i + 1, j, k + 1) + VY(i + 1, j + 1, k + 1)) * a._dy;
        const double dzi = (-VZ(i + 1, j + 1, k) + VZ(i + 1, j + 1, k + 1)) * a._dz;
        const double divV = valid ? dxi + dyi + dzi : 0.0;
        a.f.divV[c] = divV;
        if (FULL) {
            const double _Kdt = 1.0 / (a.Kc[c] * a.dt), _Gdt = 1.0 / (a.Gc[c] * a.dt), _dt = 1.0 / a.dt;
            const double P = a.theta[c], P0 = a.f.P0[c];
            const double rhs = -divV + (a.f.Q[c] * _dt);
            a.f.RP[c] = fma(-(P - P0), _Kdt, rhs);
            double et = -INFINITY;
            for (int kk = k - 1; kk <= k + 1; kk++) {
                const int kc = clampi(kk, 0, nz - 1);
                for (int jj = j - 1; jj <= j + 1; jj++) {
                    const int jc = clampi(jj, 0, ny - 1);
                    for (int ii = i - 1; ii <= i + 1; ii++) {
                        const double v = C3(a.f.eta, clampi(ii, 0, nx - 1), jc, kc);
                        if (v > et) et = v;
                    }
                }
            }
            const_cast<double *>(a.etatau)[c] = et;
            const double psi = 1.0 / (1.0 / et + _Gdt) * a.r / a.theta_dtau;
            a.theta[c] = (fma(P0, _Kdt, rhs) * psi + P) / (1.0 + _Kdt * psi);
            if (a.rho) a.f.fz[c] = vs3_rhog(a, i, j, k);
        }
        if (valid) {
            const double d3 = divV * (1.0 / 3.0);      // ∇V[i, j, k] * inv(3)
            a.f.exx[c] = dxi - d3;
            a.f.eyy[c] = dyi - d3;
            a.f.ezz[c] = dzi - d3;
        }
        if (FULL) vs3_visc_at(a, i, j, k, a.eta_out);
    }
    if (fl & VS3_YZ) EYZ(a.f.eyz, i, j, k) = 0.5 * (a._dz * (VY(i + 1, j, k + 1) - VY(i + 1, j, k)) + a._dy * (VZ(i + 1, j + 1, k) - VZ(i + 1, j, k)));
    if (fl & VS3_XZ) EXZ(a.f.exz, i, j, k) = 0.5 * (a._dz * (VX(i, j + 1, k + 1) - VX(i, j + 1, k)) + a._dx * (VZ(i + 1, j + 1, k) - VZ(i, j + 1, k)));
    if (fl & VS3_XY) EXY(a.f.exy, i, j, k) = 0.5 * (a._dy * (VX(i, j + 1, k + 1) - VX(i, j, k + 1)) + a._dx * (VY(i + 1, j, k + 1) - VY(i, j, k + 1)));
}

// Stencil tables of src/stokes/StressKernels.jl:604-668 for the edge families T = 0 (yz), 1 (xz), 2 (xy), as the unmasked 3D driver has them: entries pick the
// clamped index {0: n-1, 1: n, 2: n+1} per direction, in the reference's order of summation
__host__ __device__ constexpr int vs3_cen(int t, int q, int d)
{
    constexpr int T[3][4][3] = {
        {{1, 0, 0}, {1, 1, 0}, {1, 0, 1}, {1, 1, 1}},
        {{0, 1, 0}, {1, 1, 0}, {0, 1, 1}, {1, 1, 1}},
        {{0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}}};
    return T[t][q][d];
}
__host__ __device__ constexpr int vs3_oth(int t, int s, int q, int d)
{
    constexpr int T[3][3][4][3] = {
        {{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, {{1, 0, 1}, {2, 0, 1}, {1, 1, 1}, {2, 1, 1}}, {{1, 1, 0}, {2, 1, 0}, {1, 1, 1}, {2, 1, 1}}},
        {{{0, 1, 1}, {1, 1, 1}, {1, 2, 1}, {0, 2, 1}}, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, {{1, 1, 0}, {1, 2, 0}, {1, 1, 1}, {1, 2, 1}}},
        {{{0, 1, 1}, {1, 1, 1}, {0, 1, 2}, {1, 1, 2}}, {{1, 0, 1}, {1, 1, 1}, {1, 0, 2}, {1, 1, 2}}, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}}};
    return T[t][s][q][d];
}

// update_stresses_center_vertex! 3D (variational_stokes/StressKernels.jl:207-427) -- one edge family at a node inside its array: the return mapping of the
// unmasked kernel at a valid edge, τ = 0 at an invalid one (ε_pl and λv are left)
template <int T, bool SOFT>
__device__ __forceinline__ void vs3_edge_at(const Vs3Args &a, const int i, const int j, const int k, const int ci[3], const int cj[3], const int ck[3], const bool valid)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const int n1 = nx + (T != 0), n2 = ny + (T != 1);
    const i64 v = i + (i64)n1 * (j + (i64)n2 * k);
    if (!valid) { a.tnew[T][v] = 0.0; return; }
    i64 oc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) oc[q] = ci[vs3_cen(T, q, 0)] + (i64)nx * (cj[vs3_cen(T, q, 1)] + (i64)ny * ck[vs3_cen(T, q, 2)]);
#define AVC(A) (0.25 * ((A)[oc[0]] + (A)[oc[1]] + (A)[oc[2]] + (A)[oc[3]]))
    const double etav = 4 / (1 / a.f.eta[oc[0]] + 1 / a.f.eta[oc[1]] + 1 / a.f.eta[oc[2]] + 1 / a.f.eta[oc[3]]);
    const double Pv = AVC(a.theta);
    const double EIIv = SOFT ? AVC(a.f.EII_pl) : 0.0;
    double eij[6] = {AVC(a.f.exx), AVC(a.f.eyy), AVC(a.f.ezz), 0, 0, 0};
    double tij[6] = {AVC(a.f.txx), AVC(a.f.tyy), AVC(a.f.tzz), 0, 0, 0};
    double toij[6] = {AVC(a.f.toxx), AVC(a.f.toyy), AVC(a.f.tozz), 0, 0, 0};
#undef AVC
    const double *const esh[3] = {a.f.eyz, a.f.exz, a.f.exy}, *const tsh[3] = {a.f.tyz, a.f.txz, a.f.txy}, *const tosh[3] = {a.f.toyz, a.f.toxz, a.f.toxy};
#pragma unroll
    for (int s = 0; s < 3; s++) {
        if (s == T) { eij[3 + s] = esh[s][v]; tij[3 + s] = tsh[s][v]; toij[3 + s] = tosh[s][v]; continue; }
        const int m1 = nx + (s != 0), m2 = ny + (s != 1);
        i64 o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = ci[vs3_oth(T, s, q, 0)] + (i64)m1 * (cj[vs3_oth(T, s, q, 1)] + (i64)m2 * ck[vs3_oth(T, s, q, 2)]);
        eij[3 + s] = 0.25 * (esh[s][o[0]] + esh[s][o[1]] + esh[s][o[2]] + esh[s][o[3]]);
        tij[3 + s] = 0.25 * (tsh[s][o[0]] + tsh[s][o[1]] + tsh[s][o[2]] + tsh[s][o[3]]);
        toij[3 + s] = 0.25 * (tosh[s][o[0]] + tosh[s][o[1]] + tosh[s][o[2]] + tosh[s][o[3]]);
    }
    const double *const phsh[3] = {a.f.phase_yz, a.f.phase_xz, a.f.phase_xy};
    double *const eplsh[3] = {a.f.eplyz, a.f.eplxz, a.f.eplxy};
    const double *rv = phsh[T] + (i64)np * v;
    bool is_pl; double eta_reg;
    plastic_params<0>(a.rh, rv, is_pl, eta_reg);
    const double _Gdt = 1.0 / (ratio_avg<true>(a.rh.G, rv, np) * a.dt);
    const double Kv = ratio_avg<true>(a.rh.Kb, rv, np);
    const double dtr = 1.0 / (a.theta_dtau + etav * _Gdt + 1.0);
    double d[6], tt[6];
#pragma unroll
    for (int s = 0; s < 6; s++) { d[s] = dev_stress_inc(tij[s], toij[s], etav, eij[s], _Gdt, dtr); tt[s] = tij[s] + d[s]; }
    const double tIIv = sinv3(tt);
    double dQdt[6], dQdP, dFdP;
    plastic_grad<3, 6, 0>(a.rh, rv, tt, dQdt, dQdP, dFdP);
    const double vol = isinf(Kv) ? 0.0 : Kv * a.dt * dFdP * dQdP;
    const double F = yield_F<SOFT, 0>(a.rh, rv, Pv, tIIv, EIIv);
    constexpr int own = 3 + T;
    if (is_pl && tIIv != 0.0 && F > 0) {
        const double l = (1.0 - a.rel) * a.lamv[T][v] + a.rel * (fmax(F, 0.0) / (etav * dtr + eta_reg + vol));
        a.lamv[T][v] = l;
        const double epl = l * dQdt[own];
        a.tnew[T][v] = tij[own] + fma(-(2.0 * etav * epl), dtr, d[own]);
        eplsh[T][v] = epl;
    } else {
        a.tnew[T][v] = tij[own] + d[own];
        eplsh[T][v] = 0.0;
    }
}

// the centre block (StressKernels.jl:429-505): a valid centre as the unmasked kernel; an invalid one zeroes Pr_c, η_vep, ε_vol_pl, the six τ centre arrays and the six
// entries of @plastic_strain -- for the shear entries the EDGE arrays at the centre's own index -- and leaves τII.  Runs after the edge blocks of the same index.
template <bool SOFT>
__device__ __forceinline__ void vs3_centre_at(const Vs3Args &a, const int i, const int j, const int k, const bool valid)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const i64 c = i + (i64)nx * (j + (i64)ny * k);
    double *const tw[6] = {a.cnew[0], a.cnew[1], a.cnew[2], a.f.tyz_c, a.f.txz_c, a.f.txy_c};
    if (!valid) {
        a.f.P[c] = 0.0; a.f.eta_vep[c] = 0.0; a.f.evol_pl[c] = 0.0;
#pragma unroll
        for (int s = 0; s < 6; s++) tw[s][c] = 0.0;
        a.f.eplxx[c] = 0.0; a.f.eplyy[c] = 0.0; a.f.eplzz[c] = 0.0;
        EYZ(a.f.eplyz, i, j, k) = 0.0; EXZ(a.f.eplxz, i, j, k) = 0.0; EXY(a.f.eplxy, i, j, k) = 0.0;
        return;
    }
    const double *rc = a.f.phase_c + (i64)np * c;
    const double _Gdt = 1.0 / (ratio_avg<true>(a.rh.G, rc, np) * a.dt);
    bool is_pl; double eta_reg;
    plastic_params<0>(a.rh, rc, is_pl, eta_reg);
    const double K = ratio_avg<true>(a.rh.Kb, rc, np);
    const double e = a.f.eta[c];
    const double dtr = 1.0 / (a.theta_dtau + e * _Gdt + 1.0);
    double eij[6] = {a.f.exx[c], a.f.eyy[c], a.f.ezz[c], 0, 0, 0};
    // _av_yz / _av_xz / _av_xy = 0.25 * mysum (MiniKernels.jl): s = 0.0, then k-outer, j, i-inner adds
    eij[3] = 0.25 * ((((0.0 + EYZ(a.f.eyz, i, j, k)) + EYZ(a.f.eyz, i, j + 1, k)) + EYZ(a.f.eyz, i, j, k + 1)) + EYZ(a.f.eyz, i, j + 1, k + 1));
    eij[4] = 0.25 * ((((0.0 + EXZ(a.f.exz, i, j, k)) + EXZ(a.f.exz, i + 1, j, k)) + EXZ(a.f.exz, i, j, k + 1)) + EXZ(a.f.exz, i + 1, j, k + 1));
    eij[5] = 0.25 * ((((0.0 + EXY(a.f.exy, i, j, k)) + EXY(a.f.exy, i + 1, j, k)) + EXY(a.f.exy, i, j + 1, k)) + EXY(a.f.exy, i + 1, j + 1, k));
    const double *const tc[6] = {a.f.txx, a.f.tyy, a.f.tzz, a.f.tyz_c, a.f.txz_c, a.f.txy_c};
    const double *const toc[6] = {a.f.toxx, a.f.toyy, a.f.tozz, a.f.toyz_c, a.f.toxz_c, a.f.toxy_c};
    double tij[6], d[6], tt[6];
#pragma unroll
    for (int s = 0; s < 6; s++) {
        tij[s] = tc[s][c];
        const double to = toc[s][c];
        d[s] = (-(tij[s] - to) * e * _Gdt - tij[s] + 2.0 * e * eij[s]) * dtr;
        tt[s] = tij[s] + d[s];
    }
    double tII;
    {
        double q6[6];
#pragma unroll
        for (int s = 0; s < 6; s++) q6[s] = d[s] + tij[s];
        tII = sinv3(q6);
    }
    double dQdt[6], dQdP, dFdP;
    plastic_grad<3, 6, 0>(a.rh, rc, tt, dQdt, dQdP, dFdP);
    const double vol = isinf(K) ? 0.0 : K * a.dt * dFdP * dQdP;
    const double Pr = a.theta[c];
    const double F = yield_F<SOFT, 0>(a.rh, rc, Pr, tII, SOFT ? a.f.EII_pl[c] : 0.0);
    double l = a.lam[c];
    if (is_pl && tII != 0.0 && F > 0) {
        l = (1.0 - a.rel) * l + a.rel * (fmax(F, 0.0) / (e * dtr + eta_reg + vol));
        a.lam[c] = l;
        double epl[6];
#pragma unroll
        for (int s = 0; s < 6; s++) { epl[s] = l * dQdt[s]; d[s] = d[s] - 2.0 * e * epl[s] * dtr; tij[s] = d[s] + tij[s]; }
        a.f.evol_pl[c] = -l * dQdP;
#pragma unroll
        for (int s = 0; s < 6; s++) tw[s][c] = tij[s];
        a.f.eplxx[c] = epl[0]; a.f.eplyy[c] = epl[1]; a.f.eplzz[c] = epl[2];
        tII = sinv3(tij);
    } else {
        a.f.evol_pl[c] = 0.0;
#pragma unroll
        for (int s = 0; s < 6; s++) tw[s][c] = d[s] + tij[s];
        a.f.eplxx[c] = 0.0; a.f.eplyy[c] = 0.0; a.f.eplzz[c] = 0.0;
    }
    a.f.tII[c] = tII;
    a.f.eta_vep[c] = tII * 0.5 * (1.0 / sinv3(eij));
    a.f.P[c] = Pr - (isinf(K) ? 0.0 : K * a.dt * l * dQdP);
}

// one thread per node of the ni .+ 1 box: the three edge families, then the centre of the same index.  PART: bit T = edge family T, bit 3 = the centres.  One launch
// does it all (PART = 15) unless a phase has a softening law: with all four blocks inlined that instantiation put its argument struct into scratch memory (3136 bytes per
// lane), so the softening form runs as four launches of one block each, the centres last (their zero of ε_pl on the edges wins, as in the single launch)
template <bool SOFT, int PART>
__global__ __launch_bounds__(256) void k_vs3_stress(const Vs3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    NODE3(nx + 1, ny + 1)
    const unsigned char fl = N3(a.flags, i, j, k);
    const int ci[3] = {clampi(i - 1, 0, nx - 1), clampi(i, 0, nx - 1), clampi(i + 1, 0, nx - 1)};
    const int cj[3] = {clampi(j - 1, 0, ny - 1), clampi(j, 0, ny - 1), clampi(j + 1, 0, ny - 1)};
    const int ck[3] = {clampi(k - 1, 0, nz - 1), clampi(k, 0, nz - 1), clampi(k + 1, 0, nz - 1)};
    if ((PART & 1) && i < nx) vs3_edge_at<0, SOFT>(a, i, j, k, ci, cj, ck, (fl & VS3_YZ) != 0);
    if ((PART & 2) && j < ny) vs3_edge_at<1, SOFT>(a, i, j, k, ci, cj, ck, (fl & VS3_XZ) != 0);
    if ((PART & 4) && k < nz) vs3_edge_at<2, SOFT>(a, i, j, k, ci, cj, ck, (fl & VS3_XY) != 0);
    if ((PART & 8) && i < nx && j < ny && k < nz) vs3_centre_at<SOFT>(a, i, j, k, (fl & VS3_C) != 0);
}

// The masked momentum kernel, one thread per cell.  The masked 2D compute_V! (variational_stokes/VelocityKernels.jl:355-399) one dimension up, on the index triples of
// the unmasked 3D kernel (src/stokes/VelocityKernels.jl:215-238): every operand is multiplied by the ϕ member of its own location at its own index, ητ is unmasked;
// term order τ normal, τ shear, τ shear, -∇P, -body force; no free-surface term.  An invalid velocity node zeroes the residual and the velocity.
__global__ __launch_bounds__(256) void k_vs3_velocity(const Vs3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    NODE3(nx, ny)
    const double *__restrict__ P = a.f.P, *__restrict__ et = a.etatau;
    const double *__restrict__ pc = a.phi.center, *__restrict__ pyz = a.phi.yz, *__restrict__ pxz = a.phi.xz, *__restrict__ pxy = a.phi.xy;
    const double *__restrict__ tyz = a.f.tyz, *__restrict__ txz = a.f.txz, *__restrict__ txy = a.f.txy;
    double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy, *__restrict__ Vz = a.f.Vz;
    const double edt = a.eta_dtau;
    const i64 c = i + (i64)nx * (j + (i64)ny * k);
    const double p0 = pc[c];
#define MYZ(i_, j_, k_) (EYZ(tyz, i_, j_, k_) * EYZ(pyz, i_, j_, k_))
#define MXZ(i_, j_, k_) (EXZ(txz, i_, j_, k_) * EXZ(pxz, i_, j_, k_))
#define MXY(i_, j_, k_) (EXY(txy, i_, j_, k_) * EXY(pxy, i_, j_, k_))
    if (i < nx - 1) {
        double v = 0.0, R = 0.0;
        if (N3(a.flags, i + 1, j, k) & VS3_VX) {
            const i64 c1 = c + 1;
            const double p1 = pc[c1];
            const double dT = (-(a.f.txx[c] * p0) + a.f.txx[c1] * p1) * a._dx;
            const double dS1 = (-MXY(i + 1, j, k) + MXY(i + 1, j + 1, k)) * a._dy;
            const double dS2 = (-MXZ(i + 1, j, k) + MXZ(i + 1, j, k + 1)) * a._dz;
            const double dP = (-(P[c] * p0) + P[c1] * p1) * a._dx;
            const double av = (a.f.fx[c] * p0 + a.f.fx[c1] * p1) * 0.5;
            R = dT + dS1 + dS2 - dP - av;
            v = VX(i + 1, j + 1, k + 1) + R * edt / ((et[c] + et[c1]) * 0.5);
        }
        a.f.Rx[i + (i64)(nx - 1) * (j + (i64)ny * k)] = R;
        VX(i + 1, j + 1, k + 1) = v;
    }
    if (j < ny - 1) {
        double v = 0.0, R = 0.0;
        if (N3(a.flags, i, j + 1, k) & VS3_VY) {
            const i64 c1 = c + nx;
            const double p1 = pc[c1];
            const double dT = (-(a.f.tyy[c] * p0) + a.f.tyy[c1] * p1) * a._dy;
            const double dS1 = (-MXY(i, j + 1, k) + MXY(i + 1, j + 1, k)) * a._dx;
            const double dS2 = (-MYZ(i, j + 1, k) + MYZ(i, j + 1, k + 1)) * a._dz;
            const double dP = (-(P[c] * p0) + P[c1] * p1) * a._dy;
            const double av = (a.f.fy[c] * p0 + a.f.fy[c1] * p1) * 0.5;
            R = dT + dS1 + dS2 - dP - av;
            v = VY(i + 1, j + 1, k + 1) + R * edt / ((et[c] + et[c1]) * 0.5);
        }
        a.f.Ry[i + (i64)nx * (j + (i64)(ny - 1) * k)] = R;
        VY(i + 1, j + 1, k + 1) = v;
    }
    if (k < nz - 1) {
        double v = 0.0, R = 0.0;
        if (N3(a.flags, i, j, k + 1) & VS3_VZ) {
            const i64 c1 = c + (i64)nx * ny;
            const double p1 = pc[c1];
            const double dT = (-(a.f.tzz[c] * p0) + a.f.tzz[c1] * p1) * a._dz;
            const double dS1 = (-MXZ(i, j, k + 1) + MXZ(i + 1, j, k + 1)) * a._dx;
            const double dS2 = (-MYZ(i, j, k + 1) + MYZ(i, j + 1, k + 1)) * a._dy;
            const double dP = (-(P[c] * p0) + P[c1] * p1) * a._dz;
            const double av = (a.f.fz[c] * p0 + a.f.fz[c1] * p1) * 0.5;
            R = dT + dS1 + dS2 - dP - av;
            v = VZ(i + 1, j + 1, k + 1) + R * edt / ((et[c] + et[c1]) * 0.5);
        }
        a.f.Rz[c] = R;
        VZ(i + 1, j + 1, k + 1) = v;
    }
#undef MYZ
#undef MXZ
#undef MXY
}

// K, G averaged over the phases of a cell once per solve (compute_P!, phase form); rho: compute_ρg!(ρg, phase_ratios, rheology, args) (Stokes3D.jl:73); elin: the
// phase viscosity of the linear laws with the air correction
__global__ __launch_bounds__(256) void k_vs3_phase_avg(double *__restrict__ Kc, double *__restrict__ Gc, const Vs3Args a, const bool rho, double *__restrict__ elin)
{
    const int nx = a.nx, ny = a.ny;
    NODE3(nx, ny)
    const i64 c = i + (i64)nx * (j + (i64)ny * k);
    const double *r = a.f.phase_c + (i64)a.rh.nphase * c;
    if (elin) elin[c] = vs3_phase_viscosity(a.rh, r, a.air, 0.0, 0.0, 0.0, true);
    Kc[c] = ratio_avg<true>(a.rh.Kb, r, a.rh.nphase);
    Gc[c] = ratio_avg<true>(a.rh.G, r, a.rh.nphase);
    if (rho) a.f.fz[c] = vs3_rhog(a, i, j, k);
}
#undef C3
#undef N3
#undef VX
#undef VY
#undef VZ

// what the 3D variational driver and its kernel entry points refuse (status JRX_ERR_ARG, each named).  jrx_vep3d_params carries scalar spacings only: a non-uniform
// Geometry cannot reach the library and is refused by the binding
jrx_status vs3_check(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const jrx_rheology *rh, const jrx_vep3d_params *p, int air_phase, bool solver = true)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !rh || !p) return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: null argument");
    JRX_TRY(jrx_check_device(h));
    if (p->nx < 3 || p->ny < 3 || p->nz < 3) return jrx_fail(h, JRX_ERR_ARG, "3D Stokes needs at least 3 cells per dimension");
    if ((double)(p->nx + 2) * (double)(p->ny + 2) * (double)(p->nz + 2) >= 536870912.0)
        return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: local block too large (every array must stay below 4 GiB)");
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
    if (air_phase < 0 || air_phase > rh->nphase) return jrx_fail(h, JRX_ERR_ARG, "air_phase must be in 0..nphase (0: none)");
    if (!solver) return JRX_OK;      // compute_viscosity! is cell by cell
    if (!(p->_dx > 0.0) || !(p->_dy > 0.0) || !(p->_dz > 0.0) || std::isinf(p->_dx) || std::isinf(p->_dy) || std::isinf(p->_dz))
        return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: non-uniform spacing is not built (the inverse spacings _dx, _dy, _dz must be positive scalars)");
    if (jrx_comm_active(h)) return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: a communicator of more than one rank is not built (single block only)");
    for (int q = 0; q < rh->nphase; q++)
        if (rh->is_pl[q] != 0 && rh->is_pl[q] != 1) return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: DruckerPragerCap (phase %d) is not built", q);
    if (!phi) return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: null rock ratio");
    if (!phi->center || !phi->vertex || !phi->Vx || !phi->Vy || !phi->Vz || !phi->yz || !phi->xz || !phi->xy)
        return jrx_fail(h, JRX_ERR_ARG, "3D variational Stokes: a member of the rock ratio is NULL");
    return JRX_OK;
}

Vs3Args vs3_make(const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const jrx_rheology *rh, const jrx_vep3d_params *p, int air_phase)
{
    Vs3Args a;
    memset(&a, 0, sizeof(a));
    a.f = *f; a.rh = *rh;
    if (phi) a.phi = *phi;
    a._dx = p->_dx; a._dy = p->_dy; a._dz = p->_dz; a.dt = p->dt; a.r = p->r; a.theta_dtau = p->theta_dtau; a.eta_dtau = p->eta_dtau;
    a.rel = 0.2;      // relλ is the literal 0.2 in the 3D driver (Stokes3D.jl:137)
    a.nu = p->viscosity_relaxation; a.cut_lo = p->cutoff_lo; a.cut_hi = p->cutoff_hi;
    a.nx = (int)p->nx; a.ny = (int)p->ny; a.nz = (int)p->nz; a.air = air_phase;
    a.soft = mat_has_softening(rh);
    a.tg = p->T_ghosted != 0;
    a.vfields = mat_viscosity_reads_fields(rh); a.vinv = mat_viscosity_reads_invariant(rh); a.vtau = true;
    return a;
}

// the byte flags of a call: behind `doubles` doubles of the library scratch
jrx_status vs3_flags(jrx_handle *h, Vs3Args &a, size_t doubles)
{
    const size_t nv = (size_t)(a.nx + 1) * (a.ny + 1) * (a.nz + 1);
    JRX_TRY(jrx_ensure_etatau(h, doubles + (nv + 7) / 8));
    unsigned char *fl = reinterpret_cast<unsigned char *>(h->etatau + doubles);
    hipLaunchKernelGGL(k_vs3_flags, GRID3(a.nx + 1, a.ny + 1, a.nz + 1), dim3(256), 0, h->stream, fl, a.phi, a.nx, a.ny, a.nz);
    JRX_LAUNCH_CHECK(h);
    a.flags = fl;
    return JRX_OK;
}

void vs3_launch_stress(const Vs3Args &a, hipStream_t s)
{
    const dim3 gv = GRID3(a.nx + 1, a.ny + 1, a.nz + 1);
    if (!a.soft) { hipLaunchKernelGGL((k_vs3_stress<false, 15>), gv, dim3(256), 0, s, a); return; }
    hipLaunchKernelGGL((k_vs3_stress<true, 1>), gv, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_vs3_stress<true, 2>), gv, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_vs3_stress<true, 4>), gv, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_vs3_stress<true, 8>), gv, dim3(256), 0, s, a);
}

}   // namespace

extern "C" {

jrx_status jrx_vep3d_compute_viscosity_air(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rheology *rh, const jrx_vep3d_params *p, double nu,
                                           int32_t air_phase, int32_t tauII)
{
    JRX_TRY(vs3_check(h, f, nullptr, rh, p, air_phase, false));
    if (!f->eta || !f->phase_c) return jrx_fail(h, JRX_ERR_ARG, "compute_viscosity!: η or the phase ratios are NULL");
    if (mat_viscosity_reads_invariant(rh)) {
        const void *need[] = {f->exx, f->eyy, f->ezz, f->eyz, f->exz, f->exy, f->txx, f->tyy, f->tzz, f->tyz, f->txz, f->txy, f->P};
        for (const void *q : need)
            if (!q) return jrx_fail(h, JRX_ERR_ARG, "compute_viscosity!: a power-law creep reads stokes.ε / stokes.τ and P");
    } else if (mat_viscosity_reads_fields(rh) && !f->P) return jrx_fail(h, JRX_ERR_ARG, "compute_viscosity!: the creep law reads P");
    Vs3Args a = vs3_make(f, nullptr, rh, p, air_phase);
    a.nu = nu; a.vtau = tauII != 0;
    hipLaunchKernelGGL(k_vs3_visc, GRID3(a.nx, a.ny, a.nz), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vs3d_strain_rates(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const jrx_vep3d_params *p)
{
    jrx_rheology one;
    memset(&one, 0, sizeof(one));
    one.nphase = 1;
    JRX_TRY(vs3_check(h, f, phi, &one, p, 0));
    const void *req[] = {f->divV, f->Vx, f->Vy, f->Vz, f->exx, f->eyy, f->ezz, f->eyz, f->exz, f->exy};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "compute_strain_rate!: a required field pointer is NULL");
    Vs3Args a = vs3_make(f, phi, &one, p, 0);
    JRX_TRY(vs3_flags(h, a, 0));
    hipLaunchKernelGGL(k_vs3_pre<false>, GRID3(a.nx + 1, a.ny + 1, a.nz + 1), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vs3d_update_stresses(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const double *theta, double *lambda,
                                    double *const lambda_v[3], const jrx_rheology *rh, const jrx_vep3d_params *p)
{
    JRX_TRY(vs3_check(h, f, phi, rh, p, 0));
    if (!theta || !lambda || !lambda_v || !lambda_v[0] || !lambda_v[1] || !lambda_v[2]) return jrx_fail(h, JRX_ERR_ARG, "θ / λ / λv is NULL");
    const void *req[] = {f->P, f->exx, f->eyy, f->ezz, f->eyz, f->exz, f->exy, f->eplxx, f->eplyy, f->eplzz, f->eplyz, f->eplxz, f->eplxy, f->txx, f->tyy, f->tzz,
                         f->tyz, f->txz, f->txy, f->tyz_c, f->txz_c, f->txy_c, f->tII, f->toxx, f->toyy, f->tozz, f->toyz, f->toxz, f->toxy, f->toyz_c, f->toxz_c,
                         f->toxy_c, f->eta, f->eta_vep, f->EII_pl, f->evol_pl, f->phase_c, f->phase_yz, f->phase_xz, f->phase_xy};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "update_stresses_center_vertex!: a required field pointer is NULL");
    const EdgeN ne = edge_counts(p->nx, p->ny, p->nz);
    const size_t n = (size_t)p->nx * p->ny * p->nz, nedge = (size_t)(ne.yz + ne.xz + ne.xy);
    Vs3Args a = vs3_make(f, phi, rh, p, 0);
    JRX_TRY(vs3_flags(h, a, nedge + 3 * n));
    hipStream_t s = h->stream;
    a.theta = const_cast<double *>(theta); a.lam = lambda;
    for (int t = 0; t < 3; t++) a.lamv[t] = lambda_v[t];
    // second sets of the six arrays other nodes read while they are written (the launch writes every entry of them), copied back behind the launch
    a.tnew[0] = h->etatau; a.tnew[1] = a.tnew[0] + ne.yz; a.tnew[2] = a.tnew[1] + ne.xz;
    a.cnew[0] = a.tnew[2] + ne.xy; a.cnew[1] = a.cnew[0] + n; a.cnew[2] = a.cnew[1] + n;
    vs3_launch_stress(a, s);
    JRX_LAUNCH_CHECK(h);
    double *const dst[6] = {f->tyz, f->txz, f->txy, f->txx, f->tyy, f->tzz};
    const double *const src[6] = {a.tnew[0], a.tnew[1], a.tnew[2], a.cnew[0], a.cnew[1], a.cnew[2]};
    const size_t cnt[6] = {(size_t)ne.yz, (size_t)ne.xz, (size_t)ne.xy, n, n, n};
    for (int q = 0; q < 6; q++) JRX_HIP(h, hipMemcpyAsync(dst[q], src[q], cnt[q] * sizeof(double), hipMemcpyDeviceToDevice, s));
    JRX_HIP(h, hipStreamSynchronize(s));
    return JRX_OK;
}

jrx_status jrx_vs3d_compute_V(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const double *etatau, const jrx_vep3d_params *p)
{
    jrx_rheology one;
    memset(&one, 0, sizeof(one));
    one.nphase = 1;
    JRX_TRY(vs3_check(h, f, phi, &one, p, 0));
    const void *req[] = {f->P, f->Vx, f->Vy, f->Vz, f->txx, f->tyy, f->tzz, f->tyz, f->txz, f->txy, f->fx, f->fy, f->fz, f->Rx, f->Ry, f->Rz, etatau};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "compute_V!: a required field pointer is NULL");
    Vs3Args a = vs3_make(f, phi, &one, p, 0);
    a.etatau = etatau;
    JRX_TRY(vs3_flags(h, a, 0));
    hipLaunchKernelGGL(k_vs3_velocity, GRID3(a.nx, a.ny, a.nz), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_stokes3d_vs_solve(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const jrx_rheology *rh, const jrx_vep3d_params *p,
                                 int32_t air_phase, jrx_solve_result *res)
{
    JRX_TRY(vs3_check(h, f, phi, rh, p, air_phase));
    if (!res) return jrx_fail(h, JRX_ERR_ARG, "null result");
    if (p->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    const void *req[] = {f->P, f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Vz, f->Ux, f->Uy, f->Uz, f->exx, f->eyy, f->ezz, f->eyz, f->exz, f->exy,
                         f->eplxx, f->eplyy, f->eplzz, f->eplyz, f->eplxz, f->eplxy, f->txx, f->tyy, f->tzz, f->tyz, f->txz, f->txy,
                         f->tyz_c, f->txz_c, f->txy_c, f->tII, f->toxx, f->toyy, f->tozz, f->toyz, f->toxz, f->toxy, f->toyz_c, f->toxz_c,
                         f->toxy_c, f->eta, f->eta_vep, f->EII_pl, f->evol_pl, f->EVol_pl, f->fx, f->fy, f->fz, f->RP, f->Rx, f->Ry, f->Rz,
                         f->phase_c, f->phase_yz, f->phase_xz, f->phase_xy};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "a required 3D VEP field pointer is NULL");
    const int nx = (int)p->nx, ny = (int)p->ny, nz = (int)p->nz;
    const size_t n = (size_t)nx * ny * nz;
    const EdgeN ne = edge_counts(p->nx, p->ny, p->nz);
    const size_t nedge = (size_t)(ne.yz + ne.xz + ne.xy);
    hipStream_t s = h->stream;
    // library scratch: ητ, θ, λ, K, G, the second η, the second τxx, τyy, τzz, the phase viscosity of linear laws (centres), λv and the second edge stresses, then the byte flags
    const size_t doubles = 10 * n + 2 * nedge;
    Vs3Args a = vs3_make(f, phi, rh, p, air_phase);
    JRX_TRY(vs3_flags(h, a, doubles));
    double *etatau = h->etatau, *theta = etatau + n, *lam = theta + n, *Kc = lam + n, *Gc = Kc + n, *eta2 = Gc + n;
    double *const cset[3] = {eta2 + n, eta2 + 2 * n, eta2 + 3 * n};
    double *eta_lin = cset[2] + n;
    a.etatau = etatau; a.theta = theta; a.lam = lam; a.Kc = Kc; a.Gc = Gc; a.eta_out = eta2;
    a.lamv[0] = eta_lin + n; a.lamv[1] = a.lamv[0] + ne.yz; a.lamv[2] = a.lamv[1] + ne.xz;
    a.tnew[0] = a.lamv[2] + ne.xy; a.tnew[1] = a.tnew[0] + ne.yz; a.tnew[2] = a.tnew[1] + ne.xz;
    for (int c = 0; c < 3; c++) a.cnew[c] = cset[c];
    const dim3 gv = GRID3(nx + 1, ny + 1, nz + 1), gc = GRID3(nx, ny, nz);

    JRX_HIP(h, hipMemcpyAsync(f->P0, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // @copy stokes.P0 stokes.P
    JRX_HIP(h, hipMemcpyAsync(theta, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // θ = deepcopy(stokes.P)
    JRX_HIP(h, hipMemsetAsync(lam, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(a.lamv[0], 0, nedge * sizeof(double), s));
    // (every launch of the stress kernel writes every entry of the second sets -- an invalid edge or centre its zero -- so they need no initial values)
    const bool lin = !a.vfields;
    hipLaunchKernelGGL(k_vs3_phase_avg, gc, dim3(256), 0, s, Kc, Gc, a, rh->has_density != 0, lin ? eta_lin : (double *)nullptr);      // compute_ρg! :73
    JRX_LAUNCH_CHECK(h);
    if (lin) a.eta_lin = eta_lin;
    {   // compute_viscosity!(stokes, phase_ratios, args, rheology, air_phase, viscosity_cutoff) :74 -- relaxation 1, the strain-rate invariant
        Vs3Args a0 = a;
        a0.nu = 1.0; a0.vtau = false;
        hipLaunchKernelGGL(k_vs3_visc, gc, dim3(256), 0, s, a0);
        JRX_LAUNCH_CHECK(h);
    }
    const bool ubc = p->displacement_bcs != 0;
    const i64 nvx = (i64)(nx + 1) * (ny + 2) * (nz + 2), nvy = (i64)(nx + 2) * (ny + 1) * (nz + 2), nvz = (i64)(nx + 2) * (ny + 2) * (nz + 1);
    if (ubc) {    // displacement2velocity!(stokes, dt, flow_bcs) :77
        hipLaunchKernelGGL(k_scale3, dim3(2048), dim3(256), 0, s, f->Vx, (const double *)f->Ux, nvx, f->Vy, (const double *)f->Uy, nvy, f->Vz, (const double *)f->Uz, nvz,
                           1.0 / p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    a.rho = rh->has_density && !mat_density_is_constant(rh);       // update_ρg! :106 rewrites the same values for constant densities
    jrx_stokes3d_fields g;       // what the norms' reduction reads
    memset(&g, 0, sizeof(g));
    g.Rx = f->Rx; g.Ry = f->Ry; g.Rz = f->Rz; g.RP = f->RP;
    jrx_stokes3d_params q;
    memset(&q, 0, sizeof(q));
    q.nx = nx; q.ny = ny; q.nz = nz;

    PtLog log(res, INFINITY);
    int64_t iter = 0;
    res->iter = 0; res->nchecks = 0;
    auto keep_going = [&](int64_t it) { return it < 2 || ((log.rel() > p->eps_rel && log.err() > p->eps_abs) && it <= p->iterMax); };      // :79: no iterMin
    auto swap = [](double *&x, double *&y) { double *t_ = x; x = y; y = t_; };
    auto restore = [&]() {      // an odd number of swaps: leave η, τxx, τyy, τzz and the edge stresses in the caller's arrays
        if (a.f.eta != f->eta) {
            (void)hipMemcpyAsync(f->eta, a.f.eta, n * sizeof(double), hipMemcpyDeviceToDevice, s);
            a.eta_out = a.f.eta; a.f.eta = f->eta;
        }
        if (a.f.txx != f->txx) {
            double *const dst[6] = {f->txx, f->tyy, f->tzz, f->tyz, f->txz, f->txy};
            double **const cur[6] = {&a.f.txx, &a.f.tyy, &a.f.tzz, &a.f.tyz, &a.f.txz, &a.f.txy};
            double **const alt[6] = {&a.cnew[0], &a.cnew[1], &a.cnew[2], &a.tnew[0], &a.tnew[1], &a.tnew[2]};
            const size_t cnt[6] = {n, n, n, (size_t)ne.yz, (size_t)ne.xz, (size_t)ne.xy};
            for (int c = 0; c < 6; c++) {
                (void)hipMemcpyAsync(dst[c], *cur[c], cnt[c] * sizeof(double), hipMemcpyDeviceToDevice, s);
                *alt[c] = *cur[c]; *cur[c] = dst[c];
            }
        }
    };
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    while (keep_going(iter)) {
        const int64_t it1 = iter + 1;
        const bool check = (it1 % p->nout == 0) && it1 > 1;
        hipLaunchKernelGGL(k_vs3_pre<true>, gv, dim3(256), 0, s, a);
        JRX_LAUNCH_CHECK(h);
        swap(a.f.eta, a.eta_out);
        vs3_launch_stress(a, s);
        JRX_LAUNCH_CHECK(h);
        swap(a.f.txx, a.cnew[0]); swap(a.f.tyy, a.cnew[1]); swap(a.f.tzz, a.cnew[2]);
        swap(a.f.tyz, a.tnew[0]); swap(a.f.txz, a.tnew[1]); swap(a.f.txy, a.tnew[2]);
        hipLaunchKernelGGL(k_vs3_velocity, gc, dim3(256), 0, s, a);
        JRX_LAUNCH_CHECK(h);
        iter = it1;
        // velocity2displacement!(stokes, dt) before flow_bcs! :165-167; U is only observable behind the loop: scaled where the loop can end
        const bool last = check || !keep_going(it1);
        if (last) {
            hipLaunchKernelGGL(k_scale3, dim3(2048), dim3(256), 0, s, f->Ux, (const double *)f->Vx, nvx, f->Uy, (const double *)f->Vy, nvy, f->Uz, (const double *)f->Vz, nvz, p->dt);
            JRX_LAUNCH_CHECK(h);
        }
        if (!ubc) JRX_TRY(jrx3d_bcs(h, s, f->Vx, f->Vy, f->Vz, nx, ny, nz, p->free_slip, p->no_slip, p->periodic));
        else if (last) JRX_TRY(jrx3d_bcs(h, s, f->Ux, f->Uy, f->Uz, nx, ny, nz, p->free_slip, p->no_slip, p->periodic));
        if (check) {
            JRX_TRY(jrx3d_sumsq(h, s, &g, &q));       // Ri[2:end-1, 2:end-1, 2:end-1] and RP, not restricted to valid nodes :175-181
            double ss[4];
            JRX_TRY(jrx_read_sums(h, s, ss, false));      // single block (vs3_check)
            const double den = sqrt((double)((p->nxg - 1) * (p->nyg - 1) * (p->nzg - 1)));      // a square root here, unlike the unmasked 3D driver
            const double nRx = sqrt(ss[0]) / den, nRy = sqrt(ss[1]) / den, nRz = sqrt(ss[2]) / den;
            const double nDV = sqrt(ss[3]) / (double)n;
            const double err = log.record(iter, nRx, nRy, nRz, nDV);
            if ((p->verbose && log.rel() > p->eps_rel && err > p->eps_abs) || iter == p->iterMax) log.print3d(iter, nRx, nRy, nRz, nDV);
            if (std::isnan(err)) {      // error("NaN(s)"): leave the caller's arrays consistent and the stream drained
                restore();
                return log.fail_nan(h, iter, jrx_drain_ms(s, h->ev[6], h->ev[7]));
            }
        }
    }
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    restore();
    JRX_HIP(h, hipStreamSynchronize(s));
    float ms = 0.f;
    JRX_HIP(h, hipEventElapsedTime(&ms, h->ev[6], h->ev[7]));
    // epilogue (Stokes3D.jl:210-225): compute_vorticity!, shear2center! of ε / ε_pl / Δε, accumulate_tensor!, accumulate_vol! -- the operators of the C ABI -- and τ -> τ_o
    if (f->omega_yz && f->omega_xz && f->omega_xy) JRX_TRY(jrx_compute_vorticity3d(h, f->omega_yz, f->omega_xz, f->omega_xy, f->Vx, f->Vy, f->Vz, nx, ny, nz, p->_dx, p->_dy, p->_dz));
    if (f->eyz_c && f->exz_c && f->exy_c) JRX_TRY(jrx_shear2center3d(h, f->eyz_c, f->exz_c, f->exy_c, f->eyz, f->exz, f->exy, nx, ny, nz));
    if (f->eplyz_c && f->eplxz_c && f->eplxy_c) JRX_TRY(jrx_shear2center3d(h, f->eplyz_c, f->eplxz_c, f->eplxy_c, f->eplyz, f->eplxz, f->eplxy, nx, ny, nz));
    if (f->deyz_c && f->dexz_c && f->dexy_c && f->deyz && f->dexz && f->dexy)
        JRX_TRY(jrx_shear2center3d(h, f->deyz_c, f->dexz_c, f->dexy_c, f->deyz, f->dexz, f->dexy, nx, ny, nz));
    JRX_TRY(jrx_accumulate_tensor3d(h, f->EII_pl, f->eplxx, f->eplyy, f->eplzz, f->eplyz, f->eplxz, f->eplxy, p->dt, nx, ny, nz));
    JRX_TRY(jrx_accumulate_vol(h, f->EVol_pl, f->evol_pl, p->dt, (int64_t)n));
    JRX_TRY((jrx3d_copy_old_stresses<1024>(h, s, f, nx, ny, nz)));
    JRX_HIP(h, hipStreamSynchronize(s));
    log.finish(iter, ms);
    return JRX_OK;
}

}   // extern "C"
