// stokes2d_vs.hip -- 2D variational Stokes (free surface through a rock-ratio mask ϕ) for gfx950: RockRatio update, masked kernels, driver.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/variational_stokes/Stokes2D.jl:24-314 (_solve_VS!), mask.jl:63-157 (update_rock_ratio!,
// compute_rock_ratio), :168-254 (isvalid_c, isvalid_v, isvalid_vx, isvalid_vy), MiniKernels.jl (masked differences and averages: A[I] * ϕ[I]),
// VelocityKernels.jl:6-59 (compute_∇V!, compute_strain_rate!), :332-401 (compute_V! with dt), StressKernels.jl:2-170 (update_stresses_center_vertex! 2D),
// rheology/Viscosity.jl:382-418,638-650 (compute_viscosity_kernel! with air_phase, correct_phase_ratio); compute_P!, compute_ρg! / update_ρg! and the
// epilogue are the unmasked ones of the multiphase driver (stokes2d_vep.hip).
//
// Per PT iteration, three launches as in the sibling driver: k_vs_pre (compute_maxloc!, masked ∇V, compute_P!, [update_ρg!], masked ε, update_viscosity_τII!)
// -> k_vs_stress (vertex and centre halves; the new τxx, τyy go to a second set, then swap) -> k_vs_velocity (masked compute_V!, ghosts refreshed in-kernel once
// flow_bcs! has been applied in full).  The reference updates the viscosity between the strain rates and the stress update, after compute_maxloc! has read the
// old η: the pre kernel therefore reads η from one set and writes the relaxed η to a second one (the window of compute_maxloc! reads the neighbours' old values).
// ϕ is constant during a solve: the four validity predicates are evaluated once per call into one byte per vertex index (k_vs_flags).
// Not built: non-uniform spacing, strain_increment, more than one rank, graph replay of unobserved iterations.
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_material.hpp"
#include "stokes2d_kernels.hpp"

namespace {

enum : unsigned char { VS_C = 1, VS_V = 2, VS_VX = 4, VS_VY = 8 };

struct VsArgs {
    jrx_vep2d_fields f;
    jrx_rheology rh;
    jrx_rock_ratio2d phi;
    const unsigned char *flags;      // [(nx+1) * (ny+1)]: VS_C isvalid_c(i, j), VS_V isvalid_v(i, j), VS_VX isvalid_vx(i, j), VS_VY isvalid_vy(i, j) at index i + (nx+1) j
    const double *theta, *etatau, *Kc, *Gc;
    const double *eta_lin_c, *eta_lin_v;      // linear laws: the phase viscosity of a centre / vertex, computed once per solve (nullptr: from the ratios per call)
    double *lam, *lamv;
    double *txx_out, *tyy_out;       // where the centre half writes τxx, τyy (nullptr: in place)
    double *eta_out;                 // where the pre kernel writes the relaxed η (read from f.eta)
    double _dx, _dy, dt, r, theta_dtau, eta_dtau, rel, nu, cut_lo, cut_hi, fs_dt;
    int nx, ny, air;
    unsigned fs, ns;
    bool soft, tg, vfields, vtau, rho, obs;
};

#define C2(A, i_, j_) (A)[(i_) + (i64)nx * (j_)]
#define V2(A, i_, j_) (A)[(i_) + (i64)(nx + 1) * (j_)]

// compute_rock_ratio (mask.jl:112-119) for one member of ϕ; CellArray layout, phase index fastest
__global__ __launch_bounds__(256) void k_rock_ratio(double *__restrict__ dst, const double *__restrict__ phase, int np, int air, i64 n, int clamp)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    double x = 1.0;
    if (air >= 1 && air <= np) {
        x = 1.0 - phase[(i64)np * t + (air - 1)];
        x *= x > 1.0e-5 ? 1.0 : 0.0;
    }
    if (clamp) x = fmin(fmax(x, 0.0), 1.0);
    dst[t] = x;
}

// isvalid_c / isvalid_v / isvalid_vx / isvalid_vy (mask.jl:168-254), 0-based; ϕ.Vx is (nx+1, ny), ϕ.Vy (nx, ny+1): no ghost nodes
__global__ __launch_bounds__(256) void k_vs_flags(unsigned char *__restrict__ flags, const jrx_rock_ratio2d phi, int nx, int ny)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ pvx = phi.Vx, *__restrict__ pvy = phi.Vy;
#define PVX(i_, j_) (pvx[(i_) + (i64)(nx + 1) * (j_)] > 0)
#define PVY(i_, j_) (pvy[(i_) + (i64)nx * (j_)] > 0)
    unsigned char fl = 0;
    if (i < nx && j < ny && PVX(i, j) && PVX(i + 1, j) && PVY(i, j) && PVY(i, j + 1) && phi.center[i + (i64)nx * j] > 0) fl |= VS_C;
    {
        const int j0 = min(j, ny - 1), jb = max(j - 1, 0), i0 = min(i, nx - 1), il = max(i - 1, 0);
        if (PVX(i, j0) && PVX(i, jb) && PVY(i0, j) && PVY(il, j) && phi.vertex[i + (i64)(nx + 1) * j] > 0) fl |= VS_V;
    }
    if (j < ny && PVX(i, j)) fl |= VS_VX;
    if (i < nx && PVY(i, j)) fl |= VS_VY;
#undef PVX
#undef PVY
    flags[t] = fl;
}

// compute_phase_viscosity (rheology/Viscosity.jl:599-619) of the ratios correct_phase_ratio (:638-650) leaves; air is 1-based, 0 = none.  `≈ 1` is isapprox with its
// default rtol = sqrt(eps).  The corrected ratios are formed on the fly (an indexed local array would live in scratch memory): zero for the air phase, r / Σ r of the
// others (summed in phase order) for the rest; all zero where the air ratio ≈ 1, whose phase average is inv(0)
__device__ __forceinline__ double vs_phase_viscosity(const jrx_rheology &rh, const double *r, const int air, double AII, double T, double P, bool tau)
{
    double s = 1.0;
    if (air > 0) {
        const double ra = r[air - 1];
        if (fabs(ra - 1.0) <= 1.4901161193847656e-08 * fmax(fabs(ra), 1.0)) return 1.0 / 0.0;
        s = 0.0;
        for (int q = 0; q < rh.nphase; q++) s += q == air - 1 ? 0.0 : r[q];
    }
    // every phase's law is evaluated in a loop all lanes walk together: a return from inside it (mat_phase_viscosity) indexes the table per lane, which here put the
    // whole argument struct into scratch memory (2.8 KB per lane, 25 x the kernel time).  The first phase above 0.999 wins; air = 0: the ratios as they are
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

// compute_viscosity_kernel! at a centre / a vertex (rheology/Viscosity.jl:382-418), arguments as in the unmasked driver (local_viscosity_args :513-552)
__device__ __forceinline__ double vs_visc_centre(const VsArgs &a, const i64 t)
{
    const int nx = a.nx;
    const double *rc = a.f.phase_c + (i64)a.rh.nphase * t;
    if (a.eta_lin_c) return a.eta_lin_c[t];
    if (!a.vfields) return vs_phase_viscosity(a.rh, rc, a.air, 0.0, 0.0, 0.0, a.vtau);
    const int j = (int)(t / nx), i = (int)(t - (i64)j * nx);
    const double AII = a.vtau ? mat_visc_invariant2(a.f.txx[t], a.f.tyy[t], a.f.txy_c[t]) : mat_visc_invariant2(a.f.exx[t], a.f.eyy[t], a.f.exy_c[t]);
    const double T = !a.f.T ? 0.0 : (a.tg ? a.f.T[(i + 1) + (i64)(nx + 2) * (j + 1)] : a.f.T[t]);
    return vs_phase_viscosity(a.rh, rc, a.air, AII, T, a.f.P[t], a.vtau);
}
__device__ __forceinline__ double vs_visc_vertex(const VsArgs &a, const i64 t)
{
    const int nx = a.nx, ny = a.ny;
    const double *rv = a.f.phase_v + (i64)a.rh.nphase * t;
    if (a.eta_lin_v) return a.eta_lin_v[t];
    if (!a.vfields) return vs_phase_viscosity(a.rh, rv, a.air, 0.0, 0.0, 0.0, a.vtau);
    const int j = (int)(t / (nx + 1)), i = (int)(t - (i64)j * (nx + 1));
    const int il = max(i - 1, 0), ir = min(i, nx - 1), jb = max(j - 1, 0), jt = min(j, ny - 1);
    const double AII = mat_visc_invariant2(0.0, 0.0, a.vtau ? a.f.txy[t] : a.f.exy[t]);
    const double P = 0.25 * (a.f.P[il + (i64)nx * jb] + a.f.P[ir + (i64)nx * jb] + a.f.P[il + (i64)nx * jt] + a.f.P[ir + (i64)nx * jt]);
    double T = 0.0;
    if (a.f.T && a.tg) {
        const double *q = a.f.T + i + (i64)(nx + 2) * j;
        T = 0.25 * (q[0] + q[1] + q[nx + 2] + q[nx + 3]);
    } else if (a.f.T) T = 0.25 * (a.f.T[il + (i64)nx * jb] + a.f.T[ir + (i64)nx * jb] + a.f.T[il + (i64)nx * jt] + a.f.T[ir + (i64)nx * jt]);
    return vs_phase_viscosity(a.rh, rv, a.air, AII, T, P, a.vtau);
}
// η <- clamp(ν η_phase + (1 - ν) η): thread t serves centre t and vertex t
__device__ __forceinline__ void vs_visc_at(const VsArgs &a, const i64 t, double *eta_out)
{
    if (t < (i64)a.nx * a.ny) {
        const double e = vs_visc_centre(a, t) * a.nu + a.f.eta[t] * (1.0 - a.nu);
        eta_out[t] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
    if (a.f.eta_v && t < (i64)(a.nx + 1) * (a.ny + 1)) {
        const double e = vs_visc_vertex(a, t) * a.nu + a.f.eta_v[t] * (1.0 - a.nu);
        a.f.eta_v[t] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
}
__global__ __launch_bounds__(256) void k_vs_visc(const VsArgs a) { vs_visc_at(a, (i64)blockIdx.x * blockDim.x + threadIdx.x, a.f.eta); }

// FULL: compute_maxloc!(ητ, η) of the own cell, masked compute_∇V!, compute_P! (phase form, θ; ητ in the η slot), update_ρg! (a.rho), masked compute_strain_rate!,
// update_viscosity_τII! (η from f.eta to eta_out).  !FULL: ∇V and ε alone.
template <bool FULL>
__global__ __launch_bounds__(256) void k_vs_pre(const VsArgs a, double *__restrict__ theta)
{
    const int nx = a.nx, ny = a.ny;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy;
    const unsigned char fl = a.flags[t];
#define VX(i_, j_) Vx[(i_) + (i64)(nx + 1) * (j_)]
#define VY(i_, j_) Vy[(i_) + (i64)(nx + 2) * (j_)]
    if (i < nx && j < ny) {
        const i64 c = i + (i64)nx * j;
        const bool valid = (fl & VS_C) != 0;
        const double dxi = (-VX(i, j + 1) + VX(i + 1, j + 1)) * a._dx;
        const double dyi = (-VY(i + 1, j) + VY(i + 1, j + 1)) * a._dy;
        const double divV = valid ? dxi + dyi : 0.0;
        if (!FULL || a.obs) a.f.divV[c] = divV;
        if (FULL) {
            const double _Kdt = 1.0 / (a.Kc[c] * a.dt), _Gdt = 1.0 / (a.Gc[c] * a.dt), _dt = 1.0 / a.dt;
            const double P = theta[c], P0 = a.f.P0[c];
            const double rhs = -divV + (a.f.Q[c] * _dt);
            if (a.obs) a.f.RP[c] = fma(-(P - P0), _Kdt, rhs);
            double et = -INFINITY;
            for (int jj = j - 1; jj <= j + 1; jj++) {
                const int jc = clampi(jj, 0, ny - 1);
                for (int ii = i - 1; ii <= i + 1; ii++) {
                    const double v = a.f.eta[clampi(ii, 0, nx - 1) + (i64)nx * jc];
                    if (v > et) et = v;
                }
            }
            const_cast<double *>(a.etatau)[c] = et;
            const double psi = 1.0 / (1.0 / et + _Gdt) * a.r / a.theta_dtau;
            theta[c] = (fma(P0, _Kdt, rhs) * psi + P) / (1.0 + _Kdt * psi);
            if (a.rho) a.f.fy[c] = mat_density_ratio(a.rh, a.f.phase_c + (i64)a.rh.nphase * c, !a.f.T ? 0.0 : (a.tg ? a.f.T[i + (i64)(nx + 2) * j] : a.f.T[c]), a.f.P[c]) * a.rh.gravity;
        }
        const double d3 = divV / 3;      // ∇V[i, j] / 3 (VelocityKernels.jl:44; the unmasked kernel multiplies by inv(3))
        a.f.exx[c] = valid ? dxi - d3 : 0.0;
        a.f.eyy[c] = valid ? dyi - d3 : 0.0;
    }
    a.f.exy[t] = (fl & VS_V) ? 0.5 * ((VX(i, j + 1) - VX(i, j)) * a._dy + (VY(i + 1, j) - VY(i, j)) * a._dx) : 0.0;
#undef VX
#undef VY
    if (FULL) vs_visc_at(a, t, a.eta_out);
}

// update_stresses_center_vertex! (variational_stokes/StressKernels.jl:33-89) -- vertex half at a valid vertex; same arithmetic as the unmasked kernel's
// NP > 0: the number of phases as a compile-time constant (ratios loaded in one batch into registers, phase loops unrolled), else rh.nphase
template <bool SOFT, int NP>
__device__ __forceinline__ void vs_vertex_at(const VsArgs &a, const int i, const int j)
{
    const int nx = a.nx, ny = a.ny, np = NP > 0 ? NP : a.rh.nphase;
    const int i0 = clampi(i - 1, 0, nx - 1), ic = clampi(i, 0, nx - 1), j0 = clampi(j - 1, 0, ny - 1), jc = clampi(j, 0, ny - 1);
#define AVC(A) (0.25 * (C2(A, i0, j0) + C2(A, ic, jc) + C2(A, i0, jc) + C2(A, ic, j0)))
    const double Pv = AVC(a.theta), exxv = AVC(a.f.exx), eyyv = AVC(a.f.eyy), txxv = AVC(a.f.txx), tyyv = AVC(a.f.tyy);
    const double toxxv = AVC(a.f.toxx), toyyv = AVC(a.f.toyy);
    const double EIIv = SOFT ? AVC(a.f.EII_pl) : 0.0;
#undef AVC
    const i64 v = i + (i64)(nx + 1) * j;
    double rvv[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
        for (int q = 0; q < NP; q++) rvv[q] = a.f.phase_v[(i64)NP * v + q];
    }
    const double *rv = NP > 0 ? rvv : a.f.phase_v + (i64)np * v;
    bool is_pl; double eta_reg;
    plastic_params<NP>(a.rh, rv, is_pl, eta_reg);
    const double _Gdt = 1.0 / (ratio_avg(a.rh.G, rv, np) * a.dt);
    const double Kv = ratio_avg(a.rh.Kb, rv, np);
    const double etav = 4.0 / (1.0 / C2(a.f.eta, i0, j0) + 1.0 / C2(a.f.eta, ic, jc) + 1.0 / C2(a.f.eta, i0, jc) + 1.0 / C2(a.f.eta, ic, j0));
    const double dtr = 1.0 / (a.theta_dtau + etav * _Gdt + 1.0);
    const double txy = a.f.txy[v];
    const double dxx = dev_stress_inc(txxv, toxxv, etav, exxv, _Gdt, dtr);
    const double dyy = dev_stress_inc(tyyv, toyyv, etav, eyyv, _Gdt, dtr);
    const double dxy = dev_stress_inc(txy, a.f.toxy[v], etav, a.f.exy[v], _Gdt, dtr);
    const double tt[3] = {txxv + dxx, tyyv + dyy, txy + dxy};
    const double tIIv = sinv2(dxx + txxv, dyy + tyyv, dxy + txy);
    double dQdt[3], dQdP, dFdP;
    plastic_grad<2, 3, NP>(a.rh, rv, tt, dQdt, dQdP, dFdP);
    const double vol = isinf(Kv) ? 0.0 : Kv * a.dt * dFdP * dQdP;
    const double F = yield_F<SOFT, NP>(a.rh, rv, Pv, tIIv, EIIv);
    if (is_pl && tIIv != 0.0 && F > 0) {
        const double l = fma(1.0 - a.rel, a.lamv[v], a.rel * (fmax(F, 0.0) / (etav * dtr + eta_reg + vol)));
        a.lamv[v] = l;
        const double epl = l * dQdt[2];
        a.f.txy[v] = txy + fma(-2.0 * etav * epl, dtr, dxy);
        if (a.obs) a.f.eplxy[v] = epl;
    } else {
        a.f.txy[v] = txy + dxy;
        if (a.obs) a.f.eplxy[v] = 0.0;
    }
}

// operands of the centre half, loaded before the vertex half stores anything (see stokes2d_vep.hip)
struct VsCentreOps { double e, exyc, exx, eyy, txx, tyy, txyc, toxx, toyy, toxyc, theta, lam, EII; };
template <bool SOFT>
__device__ __forceinline__ VsCentreOps vs_centre_load(const VsArgs &a, const int i, const int j)
{
    const int nx = a.nx;
    const i64 c = i + (i64)nx * j;
    VsCentreOps o;
    o.e = a.f.eta[c];
    o.exyc = (V2(a.f.exy, i, j) + V2(a.f.exy, i + 1, j) + V2(a.f.exy, i, j + 1) + V2(a.f.exy, i + 1, j + 1)) / 4;
    o.exx = a.f.exx[c]; o.eyy = a.f.eyy[c];
    o.txx = a.f.txx[c]; o.tyy = a.f.tyy[c]; o.txyc = a.f.txy_c[c];
    o.toxx = a.f.toxx[c]; o.toyy = a.f.toyy[c]; o.toxyc = a.f.toxy_c[c];
    o.theta = a.theta[c]; o.lam = a.lam[c];
    o.EII = SOFT ? a.f.EII_pl[c] : 0.0;
    return o;
}

// centre half (StressKernels.jl:92-166): valid centres as the unmasked kernel; an invalid centre zeroes τ (xx, yy, xy_c), ε_pl (xx, yy and xy at [i, j] of the
// vertex array: ε_pl[3][I...]), Pr_c, η_vep, ε_vol_pl and leaves τII
template <bool SOFT, int NP>
__device__ __forceinline__ void vs_centre_at(const VsArgs &a, const int i, const int j, const VsCentreOps &o, const bool valid)
{
    const int nx = a.nx, np = NP > 0 ? NP : a.rh.nphase;
    const i64 c = i + (i64)nx * j;
    double *__restrict__ txx_o = a.txx_out ? a.txx_out : a.f.txx, *__restrict__ tyy_o = a.tyy_out ? a.tyy_out : a.f.tyy;
    if (!valid) {
        a.f.P[c] = 0.0;
        txx_o[c] = 0.0; tyy_o[c] = 0.0; a.f.txy_c[c] = 0.0;
        if (a.obs) {
            a.f.eta_vep[c] = 0.0; a.f.evol_pl[c] = 0.0;
            a.f.eplxx[c] = 0.0; a.f.eplyy[c] = 0.0; V2(a.f.eplxy, i, j) = 0.0;
        }
        return;
    }
    double rcv[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
        for (int q = 0; q < NP; q++) rcv[q] = a.f.phase_c[(i64)NP * c + q];
    }
    const double *rc = NP > 0 ? rcv : a.f.phase_c + (i64)np * c;
    const double _Gdt = 1.0 / (ratio_avg(a.rh.G, rc, np) * a.dt);
    bool is_pl; double eta_reg;
    plastic_params<NP>(a.rh, rc, is_pl, eta_reg);
    const double K = ratio_avg(a.rh.Kb, rc, np);
    const double e = o.e;
    const double dtr = 1.0 / (a.theta_dtau + e * _Gdt + 1.0);
    const double eij[3] = {o.exx, o.eyy, o.exyc};
    double tij[3] = {o.txx, o.tyy, o.txyc};
    const double toij[3] = {o.toxx, o.toyy, o.toxyc};
    double d[3];
#pragma unroll
    for (int q = 0; q < 3; q++) d[q] = dev_stress_inc(tij[q], toij[q], e, eij[q], _Gdt, dtr);
    double tII = sinv2(d[0] + tij[0], d[1] + tij[1], d[2] + tij[2]);
    const double tt[3] = {tij[0] + d[0], tij[1] + d[1], tij[2] + d[2]};
    double dQdt[3], dQdP, dFdP;
    plastic_grad<2, 3, NP>(a.rh, rc, tt, dQdt, dQdP, dFdP);
    const double vol = isinf(K) ? 0.0 : K * a.dt * dFdP * dQdP;
    const double Pr = o.theta;
    const double F = yield_F<SOFT, NP>(a.rh, rc, Pr, tII, o.EII);
    double l = o.lam;
    if (is_pl && tII != 0.0 && F > 0) {
        l = fma(1.0 - a.rel, l, a.rel * (fmax(F, 0.0) / (e * dtr + eta_reg + vol)));
        a.lam[c] = l;
        double epl[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            epl[q] = l * dQdt[q];
            d[q] = fma(-2.0 * e * epl[q], dtr, d[q]);
            tij[q] = d[q] + tij[q];
        }
        if (a.obs) a.f.evol_pl[c] = -l * dQdP;
        txx_o[c] = tij[0]; tyy_o[c] = tij[1]; a.f.txy_c[c] = tij[2];
        if (a.obs) { a.f.eplxx[c] = epl[0]; a.f.eplyy[c] = epl[1]; }
        tII = sinv2(tij[0], tij[1], tij[2]);
    } else {
        if (a.obs) a.f.evol_pl[c] = 0.0;
        txx_o[c] = d[0] + tij[0]; tyy_o[c] = d[1] + tij[1]; a.f.txy_c[c] = d[2] + tij[2];
        if (a.obs) { a.f.eplxx[c] = 0.0; a.f.eplyy[c] = 0.0; }
    }
    if (a.obs) {
        a.f.tII[c] = tII;
        a.f.eta_vep[c] = tII * 0.5 * (1.0 / sinv2(eij[0], eij[1], eij[2]));
    }
    a.f.P[c] = Pr - (isinf(K) ? 0.0 : K * a.dt * l * dQdP);
}

// part: 1 the vertex half, 2 the centre half, 3 both in one launch (then the centre half must write τxx, τyy to a.txx_out / a.tyy_out: the vertex half of
// the neighbours averages the OLD centre stresses)
template <bool SOFT, int NP>
__global__ __launch_bounds__(256) void k_vs_stress(const VsArgs a, const int part)
{
    const int nx = a.nx;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > a.ny) return;
    const unsigned char fl = a.flags[t];
    const bool cell = i < nx && j < a.ny && (part & 2), valid = (fl & VS_C) != 0;
    VsCentreOps o = {};
    if (cell && valid) o = vs_centre_load<SOFT>(a, i, j);
    if (part & 1) {
        if (fl & VS_V) vs_vertex_at<SOFT, NP>(a, i, j);
        else a.f.txy[t] = 0.0;
    }
    if (cell) vs_centre_at<SOFT, NP>(a, i, j, o, valid);
}

// compute_V! with dt (variational_stokes/VelocityKernels.jl:332-401): masked gradients and averages (A[I] ϕ[I], MiniKernels.jl), ρg_correction with
// ρgy ϕ.center at j and min(j + 1, ny); an invalid velocity node zeroes the residual and the velocity.  BCF: as velocity2d_cell (stokes2d_kernels.hpp)
template <bool BCF>
__global__ __launch_bounds__(256) void k_vs_velocity(const VsArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const double *__restrict__ P = a.f.P, *__restrict__ txy = a.f.txy, *__restrict__ et = a.etatau;
    const double *__restrict__ pc = a.phi.center, *__restrict__ pv = a.phi.vertex;
    const double edt = a.eta_dtau;
    const i64 c = i + (i64)nx * j;
    const double p0 = pc[c];
    if (i < nx - 1) {
        const i64 q = (i + 1) + (i64)(nx + 1) * (j + 1);
        double v = 0.0, R = 0.0;
        if (a.flags[(i + 1) + (i64)(nx + 1) * j] & VS_VX) {
            const double p1 = pc[c + 1];
            const double dP = (-(P[c] * p0) + P[c + 1] * p1) * a._dx, dT = (-(a.f.txx[c] * p0) + a.f.txx[c + 1] * p1) * a._dx;
            const double dS = (-(V2(txy, i + 1, j) * V2(pv, i + 1, j)) + V2(txy, i + 1, j + 1) * V2(pv, i + 1, j + 1)) * a._dy;
            const double av = (a.f.fx[c] * p0 + a.f.fx[c + 1] * p1) * 0.5;
            R = -dP + dT + dS - av;
            v = a.f.Vx[q] + R * edt / ((et[c] + et[c + 1]) * 0.5);
        }
        if (a.obs) a.f.Rx[i + (i64)(nx - 1) * j] = R;
        a.f.Vx[q] = v;
        if (BCF) {
            if (j == 0) { if (a.fs & JRX_FACE_BOT) a.f.Vx[q - (nx + 1)] = v; else if (a.ns & JRX_FACE_BOT) a.f.Vx[q - (nx + 1)] = -v; }
            if (j == ny - 1) { if (a.fs & JRX_FACE_TOP) a.f.Vx[q + (nx + 1)] = v; else if (a.ns & JRX_FACE_TOP) a.f.Vx[q + (nx + 1)] = -v; }
        }
    }
    if (j < ny - 1) {
        const i64 q = (i + 1) + (i64)(nx + 2) * (j + 1);
        double v = 0.0, R = 0.0;
        if (a.flags[i + (i64)(nx + 1) * (j + 1)] & VS_VY) {
            const double p1 = pc[c + nx];
            const double vy0 = a.f.Vy[q];
            const double rgS = a.f.fy[c] * p0, rgN = a.f.fy[c + nx] * p1;      // j_N = min(j + 1, ny) = j + 1 here
            const double corr = (vy0 * ((rgN - rgS) * a._dy)) * 1.0 * a.fs_dt;
            const double dP = (-(P[c] * p0) + P[c + nx] * p1) * a._dy, dT = (-(a.f.tyy[c] * p0) + a.f.tyy[c + nx] * p1) * a._dy;
            const double dS = (-(V2(txy, i, j + 1) * V2(pv, i, j + 1)) + V2(txy, i + 1, j + 1) * V2(pv, i + 1, j + 1)) * a._dx;
            const double av = (rgS + rgN) * 0.5;
            R = -dP + dT + dS - av + corr;
            v = vy0 + R * edt / ((et[c] + et[c + nx]) * 0.5);
        }
        if (a.obs) a.f.Ry[c] = R;
        a.f.Vy[q] = v;
        if (BCF) {
            if (i == 0) { if (a.fs & JRX_FACE_LEFT) a.f.Vy[q - 1] = v; else if (a.ns & JRX_FACE_LEFT) a.f.Vy[q - 1] = -v; }
            if (i == nx - 1) { if (a.fs & JRX_FACE_RIGHT) a.f.Vy[q + 1] = v; else if (a.ns & JRX_FACE_RIGHT) a.f.Vy[q + 1] = -v; }
        }
    }
}

// K, G averaged over the phases of a cell once per solve (compute_P! phase form); rho: compute_ρg!(ρg[end], phase_ratios, rheology, args) (Stokes2D.jl:101)
__global__ __launch_bounds__(256) void k_vs_phase_avg(double *__restrict__ Kc, double *__restrict__ Gc, const VsArgs a, const bool rho, double *__restrict__ elc,
                                                      double *__restrict__ elv)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (elv && t < (i64)(a.nx + 1) * (a.ny + 1)) elv[t] = vs_phase_viscosity(a.rh, a.f.phase_v + a.rh.nphase * t, a.air, 0.0, 0.0, 0.0, true);
    if (t >= (i64)a.nx * a.ny) return;
    const double *r = a.f.phase_c + a.rh.nphase * t;
    if (elc) elc[t] = vs_phase_viscosity(a.rh, r, a.air, 0.0, 0.0, 0.0, true);
    Kc[t] = ratio_avg(a.rh.Kb, r, a.rh.nphase);
    Gc[t] = ratio_avg(a.rh.G, r, a.rh.nphase);
    if (rho) a.f.fy[t] = mat_density_ratio(a.rh, r, !a.f.T ? 0.0 : (a.tg ? a.f.T[(t % a.nx) + (i64)(a.nx + 2) * (t / a.nx)] : a.f.T[t]), a.f.P[t]) * a.rh.gravity;
}

// Σx² of Rx[ϕ.Vx[2:end-1, :] .> 0], Ry[ϕ.Vy[:, 2:end-1] .> 0], RP[ϕ.center .> 0] (Stokes2D.jl:255-259): partials [block][4], then k_sumsq_final
__global__ __launch_bounds__(256) void k_vs_sumsq_partial(const VsArgs a, double *__restrict__ partials)
{
    __shared__ double sm[3][4];
    const int nx = a.nx, ny = a.ny;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 stride = (i64)gridDim.x * blockDim.x, n = (i64)nx * ny;
    double s[3] = {0.0, 0.0, 0.0};
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const int j = (int)(t / nx), i = (int)(t - (i64)j * nx);
        if (i < nx - 1 && a.phi.Vx[(i + 1) + (i64)(nx + 1) * j] > 0) { const double v = a.f.Rx[i + (i64)(nx - 1) * j]; s[0] += v * v; }
        if (j < ny - 1 && a.phi.Vy[i + (i64)nx * (j + 1)] > 0) { const double v = a.f.Ry[t]; s[1] += v * v; }
        if (a.phi.center[t] > 0) { const double v = a.f.RP[t]; s[2] += v * v; }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double w = wave_sum(s[c]);
        if (lane == 0) sm[c][wave] = w;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        partials[(i64)blockIdx.x * 4 + c] = c < 3 ? (sm[c][0] + sm[c][1]) + (sm[c][2] + sm[c][3]) : 0.0;
    }
}

// post-loop epilogue (Stokes2D.jl:289-301): compute_vorticity!, shear2center! x3, accumulate_tensor!, accumulate_vol!
__device__ __forceinline__ double vs_sinv_stag(double xx, double yy, double p, double q, double r, double s)
{
    return sqrt(0.5 * (xx * xx + yy * yy) + 0.25 * (p * p + q * q + r * r + s * s));
}
__global__ __launch_bounds__(256) void k_vs_epilogue(const VsArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    if (a.f.omega_xy)
        V2(a.f.omega_xy, i, j) = 0.5 * ((-a.f.Vy[i + (i64)(nx + 2) * j] + a.f.Vy[(i + 1) + (i64)(nx + 2) * j]) * a._dx -
                                        (-a.f.Vx[i + (i64)(nx + 1) * j] + a.f.Vx[i + (i64)(nx + 1) * (j + 1)]) * a._dy);
    if (i < nx && j < ny) {
        const i64 c = i + (i64)nx * j;
#define S2C(V) (0.25 * (V2(V, i, j) + V2(V, i + 1, j) + V2(V, i, j + 1) + V2(V, i + 1, j + 1)))
        if (a.f.exy_c) a.f.exy_c[c] = S2C(a.f.exy);
        if (a.f.eplxy_c) a.f.eplxy_c[c] = S2C(a.f.eplxy);
        if (a.f.dexy_c && a.f.dexy) a.f.dexy_c[c] = S2C(a.f.dexy);
#undef S2C
        a.f.EII_pl[c] += vs_sinv_stag(a.f.eplxx[c], a.f.eplyy[c], V2(a.f.eplxy, i, j), V2(a.f.eplxy, i + 1, j), V2(a.f.eplxy, i, j + 1),
                                      V2(a.f.eplxy, i + 1, j + 1)) * a.dt;
        a.f.EVol_pl[c] += a.dt * a.f.evol_pl[c];
    }
}
#undef C2
#undef V2

// what the variational driver and its kernel entry points refuse (status JRX_ERR_ARG, each named)
jrx_status vs_check(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const jrx_rheology *rh, const jrx_vep2d_params *p, int air_phase, bool solver = true)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !rh || !p) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: null argument");
    JRX_TRY(jrx_check_device(h));
    if (p->nx < 3 || p->ny < 3) return jrx_fail(h, JRX_ERR_ARG, "2D Stokes needs at least 3 cells per dimension");
    if ((p->nx + 2) * (p->ny + 2) > (int64_t)1 << 28) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: the grid exceeds the 32-bit offsets of its kernels");
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
    if (air_phase < 0 || air_phase > rh->nphase) return jrx_fail(h, JRX_ERR_ARG, "air_phase must be in 0..nphase (0: none)");
    if (!solver) return JRX_OK;      // compute_viscosity! is node by node: no spacing, no neighbours
    for (int q = 0; q < 6; q++)
        if (p->inv_spacing[q]) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: a non-uniform Geometry (inv_spacing) is not built");
    if (p->strain_increment) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: strain_increment is not built");
    if (jrx_comm_active(h)) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: a communicator of more than one rank is not built (single block only)");
    for (int q = 0; q < rh->nphase; q++)
        if (rh->is_pl[q] != 0 && rh->is_pl[q] != 1) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: DruckerPragerCap (phase %d) is not built", q);
    if (phi && (!phi->center || !phi->vertex || !phi->Vx || !phi->Vy)) return jrx_fail(h, JRX_ERR_ARG, "variational Stokes: a member of the rock ratio is NULL");
    return JRX_OK;
}

VsArgs vs_make(const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const jrx_rheology *rh, const jrx_vep2d_params *p, int air_phase)
{
    VsArgs a;
    memset(&a, 0, sizeof(a));
    a.f = *f; a.rh = *rh;
    if (phi) a.phi = *phi;
    a._dx = p->_dx; a._dy = p->_dy; a.dt = p->dt; a.r = p->r; a.theta_dtau = p->theta_dtau; a.eta_dtau = p->eta_dtau; a.rel = p->lambda_relaxation;
    a.nu = p->viscosity_relaxation; a.cut_lo = p->cutoff_lo; a.cut_hi = p->cutoff_hi;
    a.fs_dt = p->free_surface ? p->dt : 0.0;      // dt * free_surface with a Bool: Inf * false == 0.0 in Julia
    a.nx = (int)p->nx; a.ny = (int)p->ny; a.air = air_phase;
    a.fs = p->free_slip; a.ns = p->no_slip;
    a.soft = mat_has_softening(rh);
    a.tg = p->T_ghosted != 0;
    a.vfields = mat_viscosity_reads_fields(rh); a.vtau = true;
    a.obs = true;
    return a;
}

// the byte flags of a call: behind `doubles` doubles of the library scratch
jrx_status vs_flags(jrx_handle *h, VsArgs &a, size_t doubles)
{
    const size_t nv = (size_t)(a.nx + 1) * (a.ny + 1);
    JRX_TRY(jrx_ensure_etatau(h, doubles + (nv + 7) / 8));
    unsigned char *fl = reinterpret_cast<unsigned char *>(h->etatau + doubles);
    hipLaunchKernelGGL(k_vs_flags, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, h->stream, fl, a.phi, a.nx, a.ny);
    JRX_LAUNCH_CHECK(h);
    a.flags = fl;
    return JRX_OK;
}

// the stress kernel's instantiation: softening laws take the general form, otherwise the phase count is a constant up to four (option vep3_np_const, as the sibling driver)
void vs_launch_stress(jrx_handle *h, const VsArgs &a, unsigned gv, hipStream_t s, int part)
{
    auto go = [&](auto SOFT, auto NP) { hipLaunchKernelGGL((k_vs_stress<SOFT(), NP()>), dim3(gv), dim3(256), 0, s, a, part); };
    if (a.soft) go(std::true_type{}, std::integral_constant<int, 0>{});
    else dispatch_const<0, 1, 2, 3, 4>(h->vep3_np_const && a.rh.nphase <= 4 ? a.rh.nphase : 0, [&](auto NP) { go(std::false_type{}, NP); });
}

}   // namespace

extern "C" {

jrx_status jrx_update_rock_ratio(jrx_handle *h, double *dst, const double *phase, int32_t nphase, int32_t air_phase, int64_t count, int32_t clamp)
{
    if (!h) return JRX_ERR_ARG;
    if (!dst || !phase || nphase < 1 || count < 1) return jrx_fail(h, JRX_ERR_ARG, "update_rock_ratio!: bad argument");
    JRX_TRY(jrx_check_device(h));
    hipLaunchKernelGGL(k_rock_ratio, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, dst, phase, (int)nphase, (int)air_phase, (i64)count, (int)clamp);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vep2d_compute_viscosity_air(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu,
                                           int32_t air_phase, int32_t tauII)
{
    JRX_TRY(vs_check(h, f, nullptr, rh, p, air_phase, false));
    if (!f->eta || !f->phase_c || (f->eta_v && !f->phase_v)) return jrx_fail(h, JRX_ERR_ARG, "compute_viscosity!: η or the phase ratios are NULL");
    VsArgs a = vs_make(f, nullptr, rh, p, air_phase);
    a.nu = nu; a.vtau = tauII != 0;
    hipLaunchKernelGGL(k_vs_visc, dim3((unsigned)(((p->nx + 1) * (p->ny + 1) + 255) / 256)), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vs2d_strain_rates(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const jrx_vep2d_params *p)
{
    jrx_rheology one;
    memset(&one, 0, sizeof(one));
    one.nphase = 1;
    if (!phi) return h ? jrx_fail(h, JRX_ERR_ARG, "variational Stokes: null rock ratio") : JRX_ERR_ARG;
    JRX_TRY(vs_check(h, f, phi, &one, p, 0));
    if (!f->divV || !f->Vx || !f->Vy || !f->exx || !f->eyy || !f->exy) return jrx_fail(h, JRX_ERR_ARG, "compute_strain_rate!: a required field pointer is NULL");
    VsArgs a = vs_make(f, phi, &one, p, 0);
    JRX_TRY(vs_flags(h, a, 0));
    const unsigned gv = (unsigned)(((p->nx + 1) * (p->ny + 1) + 255) / 256);
    hipLaunchKernelGGL(k_vs_pre<false>, dim3(gv), dim3(256), 0, h->stream, a, (double *)nullptr);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vs2d_update_stresses(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const double *theta, double *lambda,
                                    double *lambda_v, const jrx_rheology *rh, const jrx_vep2d_params *p)
{
    if (!phi) return h ? jrx_fail(h, JRX_ERR_ARG, "variational Stokes: null rock ratio") : JRX_ERR_ARG;
    JRX_TRY(vs_check(h, f, phi, rh, p, 0));
    if (!theta || !lambda || !lambda_v) return jrx_fail(h, JRX_ERR_ARG, "θ / λ / λv is NULL");
    const void *req[] = {f->P, f->exx, f->eyy, f->exy, f->eplxx, f->eplyy, f->eplxy, f->txx, f->tyy, f->txy, f->txy_c, f->tII, f->toxx, f->toyy, f->toxy,
                         f->toxy_c, f->eta, f->eta_vep, f->EII_pl, f->evol_pl, f->phase_c, f->phase_v};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "update_stresses_center_vertex!: a required field pointer is NULL");
    VsArgs a = vs_make(f, phi, rh, p, 0);
    a.theta = theta; a.lam = lambda; a.lamv = lambda_v;
    JRX_TRY(vs_flags(h, a, 0));
    const unsigned gv = (unsigned)(((p->nx + 1) * (p->ny + 1) + 255) / 256);
    for (int part = 1; part <= 2; part++) {      // the vertex half first: it averages the old centre stresses
        vs_launch_stress(h, a, gv, h->stream, part);
        JRX_LAUNCH_CHECK(h);
    }
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vs2d_compute_V(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const double *etatau, const jrx_vep2d_params *p)
{
    jrx_rheology one;
    memset(&one, 0, sizeof(one));
    one.nphase = 1;
    if (!phi) return h ? jrx_fail(h, JRX_ERR_ARG, "variational Stokes: null rock ratio") : JRX_ERR_ARG;
    JRX_TRY(vs_check(h, f, phi, &one, p, 0));
    const void *req[] = {f->P, f->Vx, f->Vy, f->txx, f->tyy, f->txy, f->fx, f->fy, f->Rx, f->Ry, etatau};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "compute_V!: a required field pointer is NULL");
    VsArgs a = vs_make(f, phi, &one, p, 0);
    a.etatau = etatau;
    JRX_TRY(vs_flags(h, a, 0));
    hipLaunchKernelGGL(k_vs_velocity<false>, dim3((unsigned)((p->nx * p->ny + 255) / 256)), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_stokes2d_vs_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                                 const jrx_vep2d_params *p, int32_t air_phase, jrx_solve_result *res)
{
    if (!phi) return h ? jrx_fail(h, JRX_ERR_ARG, "variational Stokes: null rock ratio") : JRX_ERR_ARG;
    JRX_TRY(vs_check(h, f, phi, rh, p, air_phase));
    if (!res) return jrx_fail(h, JRX_ERR_ARG, "null result");
    if (p->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    const void *req[] = {f->P, f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Ux, f->Uy, f->exx, f->eyy, f->exy, f->eplxx, f->eplyy, f->eplxy, f->eplxy_c,
                         f->txx, f->tyy, f->txy, f->txy_c, f->tII, f->toxx, f->toyy, f->toxy, f->toxy_c, f->eta, f->eta_vep, f->EII_pl, f->evol_pl,
                         f->EVol_pl, f->fx, f->fy, f->RP, f->Rx, f->Ry, f->phase_c, f->phase_v};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "a required VEP field pointer is NULL");
    if (mat_viscosity_reads_invariant(rh) && !f->exy_c) return jrx_fail(h, JRX_ERR_ARG, "a power-law creep needs ε.xy_c for compute_viscosity!");
    const int nx = (int)p->nx, ny = (int)p->ny;
    const size_t n = (size_t)nx * ny, nv = (size_t)(nx + 1) * (ny + 1);
    hipStream_t s = h->stream;
    // library scratch: ητ, θ, λ, K, G (centre), λv (vertex), the second sets of τxx, τyy and η, the phase viscosities of linear laws (centre, vertex), then the byte flags
    const size_t doubles = 9 * n + 2 * nv;
    VsArgs a = vs_make(f, phi, rh, p, air_phase);
    JRX_TRY(vs_flags(h, a, doubles));
    double *etatau = h->etatau, *theta = etatau + n, *lam = theta + n, *Kc = lam + n, *Gc = Kc + n, *lamv = Gc + n;
    a.theta = theta; a.etatau = etatau; a.Kc = Kc; a.Gc = Gc; a.lam = lam; a.lamv = lamv;
    a.txx_out = lamv + nv; a.tyy_out = a.txx_out + n; a.eta_out = a.tyy_out + n;
    const unsigned gv = (unsigned)((nv + 255) / 256), gc = (unsigned)((n + 255) / 256);

    JRX_HIP(h, hipMemcpyAsync(f->P0, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // @copy stokes.P0 stokes.P
    JRX_HIP(h, hipMemcpyAsync(theta, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // θ = deepcopy(stokes.P)
    JRX_HIP(h, hipMemsetAsync(lam, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(lamv, 0, nv * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxx, 0, n * sizeof(double), s));                                 // @tensor_center(ε_pl) .= 0
    JRX_HIP(h, hipMemsetAsync(f->eplyy, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxy_c, 0, n * sizeof(double), s));
    // linear laws: η of a cell / vertex depends on its (corrected) phase ratios only -- averaged once per solve, the viscosity updates then read one array instead of the ratios
    const bool lin = !a.vfields;
    double *eta_lin_c = a.eta_out + n, *eta_lin_v = eta_lin_c + n;
    hipLaunchKernelGGL(k_vs_phase_avg, dim3(lin && f->eta_v ? gv : gc), dim3(256), 0, s, Kc, Gc, a, rh->has_density != 0, lin ? eta_lin_c : (double *)nullptr,
                       lin && f->eta_v ? eta_lin_v : (double *)nullptr);      // compute_ρg!(ρg[end], ...) :101
    JRX_LAUNCH_CHECK(h);
    if (lin) { a.eta_lin_c = eta_lin_c; a.eta_lin_v = f->eta_v ? eta_lin_v : nullptr; }
    {   // compute_viscosity!(stokes, phase_ratios, args, rheology, viscosity_cutoff; air_phase) :102 -- relaxation 1, the strain-rate invariant
        VsArgs a0 = a;
        a0.nu = 1.0; a0.vtau = false;
        hipLaunchKernelGGL(k_vs_visc, dim3(gv), dim3(256), 0, s, a0);
        JRX_LAUNCH_CHECK(h);
    }
    const bool ubc = p->displacement_bcs != 0;
    if (ubc) {    // displacement2velocity!(stokes, dt, flow_bcs) :103
        hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Vx, (const double *)f->Ux, (i64)(nx + 1) * (ny + 2), f->Vy,
                           (const double *)f->Uy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, 1.0 / p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    a.rho = rh->has_density && !mat_density_is_constant(rh);       // update_ρg! :133 rewrites the same values for constant densities
    const int nblk = (int)(gc < (unsigned)kMaxRedBlocks ? gc : (unsigned)kMaxRedBlocks);

    PtLog log(res);
    int64_t iter = 0;
    auto done = [&]() { return log.rel() < p->eps_rel || log.err() < p->eps_abs; };
    auto restore = [&]() {      // an odd number of swaps: leave τxx, τyy, η in the caller's arrays
        if (a.f.txx != f->txx) {
            (void)hipMemcpyAsync(f->txx, a.f.txx, n * sizeof(double), hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(f->tyy, a.f.tyy, n * sizeof(double), hipMemcpyDeviceToDevice, s);
            a.txx_out = a.f.txx; a.tyy_out = a.f.tyy; a.f.txx = f->txx; a.f.tyy = f->tyy;
        }
        if (a.f.eta != f->eta) {
            (void)hipMemcpyAsync(f->eta, a.f.eta, n * sizeof(double), hipMemcpyDeviceToDevice, s);
            a.eta_out = a.f.eta; a.f.eta = f->eta;
        }
    };
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    while (iter <= p->iterMax) {
        if (p->iterMin < iter && done()) break;                                                  // :106
        const int64_t it1 = iter + 1;
        const bool check = (it1 % p->nout == 0) && it1 > 1;
        // can the loop stop after this iteration (a check, the last allowed one, or already converged)?  Only then are its output-only arrays stored
        const bool last = check || it1 > p->iterMax || (p->iterMin < it1 && done());
        a.obs = last || h->vep_store_all;
        if (!last && h->vep_store_all) h->stat_vep_store_all++;
        hipLaunchKernelGGL(k_vs_pre<true>, dim3(gv), dim3(256), 0, s, a, theta);
        JRX_LAUNCH_CHECK(h);
        { double *t_ = a.f.eta; a.f.eta = a.eta_out; a.eta_out = t_; }
        vs_launch_stress(h, a, gv, s, 3);
        JRX_LAUNCH_CHECK(h);
        { double *t_ = a.f.txx; a.f.txx = a.txx_out; a.txx_out = t_; }
        { double *t_ = a.f.tyy; a.f.tyy = a.tyy_out; a.tyy_out = t_; }
        // flow_bcs! applied in full by iteration 1: compute_V! refreshes the ghosts itself, except where U = V dt is observable (it copies the ghosts flow_bcs! left before)
        const bool bcf = iter >= 1 && p->periodic == 0 && !ubc && !last;
        if (bcf) hipLaunchKernelGGL(k_vs_velocity<true>, dim3(gc), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_vs_velocity<false>, dim3(gc), dim3(256), 0, s, a);
        JRX_LAUNCH_CHECK(h);
        iter = it1;
        if (last) {   // velocity2displacement!(stokes, dt) before flow_bcs! :244-246
            hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Ux, (const double *)f->Vx, (i64)(nx + 1) * (ny + 2), f->Uy,
                               (const double *)f->Vy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, p->dt);
            JRX_LAUNCH_CHECK(h);
        }
        if (ubc) {
            if (last) JRX_TRY(jrx2d_bcs(h, s, f->Ux, f->Uy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        } else if (!bcf) JRX_TRY(jrx2d_bcs(h, s, f->Vx, f->Vy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        if (check) {
            hipLaunchKernelGGL(k_vs_sumsq_partial, dim3(nblk), dim3(256), 0, s, a, h->d_partials);
            hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, s, (const double *)h->d_partials, nblk, h->d_sums);
            JRX_LAUNCH_CHECK(h);
            double ss[4];
            JRX_TRY(jrx_read_sums(h, s, ss, false));      // single block (vs_check); k_vs_sumsq_partial leaves RP in slot 2
            const double nRx = sqrt(ss[0]) / sqrt((double)((p->nxg - 2) * (p->nyg - 1)));
            const double nRy = sqrt(ss[1]) / sqrt((double)((p->nxg - 1) * (p->nyg - 2)));
            const double nDV = sqrt(ss[2]) / sqrt((double)(p->nxg * p->nyg));
            const double err = log.record(iter, nRx, nRy, nDV);
            if (p->verbose) log.print2d(iter, nRx, nRy, nDV);
            if (std::isnan(err)) {      // error("NaN(s)"): leave the caller's arrays consistent and the stream drained
                restore();
                return log.fail_nan(h, iter, jrx_drain_ms(s, h->ev[6], h->ev[7]));
            }
        }
    }
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    restore();
    a.txx_out = a.tyy_out = nullptr;
    hipLaunchKernelGGL(k_vs_epilogue, dim3(gv), dim3(256), 0, s, a);
    JRX_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(k_copy6, dim3(256), dim3(256), 0, s, f->toxx, (const double *)f->txx, (i64)n, f->toyy, (const double *)f->tyy, (i64)n,
                       f->toxy, (const double *)f->txy, (i64)nv, f->toxy_c, (const double *)f->txy_c, (i64)n, (double *)nullptr,
                       (const double *)nullptr, (i64)0, (double *)nullptr, (const double *)nullptr, (i64)0);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(s));
    float ms = 0.f;
    JRX_HIP(h, hipEventElapsedTime(&ms, h->ev[6], h->ev[7]));
    log.finish(iter, ms);
    return JRX_OK;
}

}   // extern "C"
