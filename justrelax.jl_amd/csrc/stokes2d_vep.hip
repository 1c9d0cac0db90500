// stokes2d_vep.hip -- 2D multiphase visco-elasto-plastic and single-phase non-linear pseudo-transient Stokes drivers for gfx950.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/stokes/Stokes2D.jl:577-866 (multiphase driver, config 5: shear band) and
// :345-557 (single-phase MaterialParams driver), src/stokes/StressKernels.jl:992-1302 (update_stresses_center_vertex_ps! 2D and its
// strain_increment form), :266-351 (compute_τ_nonlinear!), :379-431 (accumulate_tensor!, accumulate_vol!), PressureKernels.jl:47-106
// (compute_P! with phase ratios), rheology/Viscosity.jl:142-167,382-418,513-552,599-625 (compute_viscosity!, update_viscosity_τII!),
// rheology/StressUpdate.jl:2-57,152-176,399-410,476-495 (plastic parameters, yield function, gradients), VelocityKernels.jl:46-57
// (compute_strain_rate_from_increment!), stress_rotation_particles.jl:17-29 (vorticity), Interpolations.jl:101-114,306-311
// (center2vertex!, shear2center!), as test/test_shearband2D.jl drives them.
// Rheology table (jrx_rheology): per-phase LinearViscous η or creep law, ConstantElasticity (G, Kb), DruckerPrager_regularised
// (C, ϕ, ψ, η_vp, optional softening); densities constant (ρg given) or updated from T, P.
//
// Per PT iteration of the multiphase driver: k_vep_pre (compute_maxloc!, ∇V, θ, RP, ε) [-> k_vep_strain_inc] -> k_vep_stress2d (vertex
// and centre halves of the stress update in one launch; the new τxx, τyy go to a second set, then swap) -> k_vep_visc_velocity
// (compute_viscosity! + compute_V! of the visco-elastic path, stokes2d_kernels.hpp) -> BCs (in-kernel once applied in full).
// Launch-bound at the reference's sizes: runs of unobserved iterations replay as captured graphs.
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_material.hpp"
#include "stokes2d_kernels.hpp"

namespace {

struct VepArgs {
    jrx_vep2d_fields f;
    jrx_rheology rh;
    const double *theta, *etatau, *Kc, *Gc;
    const double *eta_lin_c, *eta_lin_v;                // linear laws: phase-averaged η at centres / vertices, computed once per solve (nullptr: from the ratios per call)
    const double *src;                                  // args.ΔT: the thermal source α_c * (ΔT * _dt) of compute_P! at the centres, constant over a solve (k_phase_avg); read by the TH forms of the pre kernels only
    double *lam, *lamv;
    double *txx_out = nullptr, *tyy_out = nullptr;      // where the centre half writes τxx, τyy (nullptr: in place)
    Sp2 sp;                                             // non-uniform grid: inverse spacing arrays (all NULL: _dx, _dy)
    double _dx, _dy, dt, r, theta_dtau, rel, nu, cut_lo, cut_hi;
    int nx, ny;
    bool soft;            // some phase has a softening law (EII_pl is then read by the yield function)
    bool si;              // strain_increment variant
    bool tg;              // args.T is the ghosted thermal.T (nx+2, ny+2): densities read it at the cell's own [i, j], unshifted (BuoyancyForces.jl:52)
    bool dtg;             // args.ΔT is the ghosted thermal.ΔT (nx+2, ny+2): compute_P! reads it at the cell's own [i, j], unshifted (PressureKernels.jl:149)
    bool vfields;         // some phase's creep law reads T, P or the invariant (visc_kind != 0)
    bool vtau;            // the viscosity is taken from the stress (update_viscosity_τII!, the in-loop form) rather than from the strain rate (compute_viscosity!)
    bool obs = true;      // the outputs nothing inside the PT loop reads -- ∇V, RP, ε_pl (3), ε_vol_pl, τII, η_vep -- are stored; the solve loop clears it on iterations whose
                          // results cannot be observed (not a norm check, not the last one): the next iteration overwrites them anyway
};

// GeoParams second_invariant_staggered: the shear slot enters as the mean of the squared vertex values
// (pinned by the extrema of test/test_shearband2D.jl:198-199: mean-then-square misses them by 2.8e-3)
__device__ __forceinline__ double sinv_stag(double xx, double yy, double a, double b, double c, double d)
{
    return sqrt(0.5 * (xx * xx + yy * yy) + 0.25 * (a * a + b * b + c * c + d * d));
}

#define C2(A, i_, j_) (A)[(i_) + (i64)nx * (j_)]
#define V2(A, i_, j_) (A)[(i_) + (i64)(nx + 1) * (j_)]

// compute_∇V! + compute_P! (phase form: K, G phase-averaged once per solve; writes θ) + compute_strain_rate!
// ML: compute_maxloc!(ητ, η) of the own cell first (clamped 3 x 3 window, same comparison order as k_maxloc) and store it: saves the
// separate launch of the launch-bound 2D loop
// RHO: update_ρg! of the own cell (args.T, args.P = stokes.P; phase-ratio density times the scalar gravity, into the last component of ρg)
// TH: the thermal form of _compute_P! (PressureKernels.jl:197-206): rhs = (-∇V + (α * (ΔT * _dt))) + (Q * _dt), the middle term read from a.src
template <bool ML, bool RHO = false, bool TH = false>
__global__ __launch_bounds__(256) void k_vep_pre(const VepArgs a, double *__restrict__ theta)
{
    const int nx = a.nx, ny = a.ny;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy;
#define VX(i_, j_) Vx[(i_) + (i64)(nx + 1) * (j_)]
#define VY(i_, j_) Vy[(i_) + (i64)(nx + 2) * (j_)]
    if (i < nx && j < ny) {
        const i64 c = i + (i64)nx * j;
        const double dxi = (-VX(i, j + 1) + VX(i + 1, j + 1)) * spc(a.sp.vx, i, a._dx);
        const double dyi = (-VY(i + 1, j) + VY(i + 1, j + 1)) * spc(a.sp.vy, j, a._dy);
        const double divV = dxi + dyi;
        if (a.obs) a.f.divV[c] = divV;
        const double _Kdt = 1.0 / (a.Kc[c] * a.dt), _Gdt = 1.0 / (a.Gc[c] * a.dt), _dt = 1.0 / a.dt;
        const double P = theta[c], P0 = a.f.P0[c];
        const double rhs = TH ? (-divV + a.src[c]) + (a.f.Q[c] * _dt) : -divV + (a.f.Q[c] * _dt);
        if (a.obs) a.f.RP[c] = fma(-(P - P0), _Kdt, rhs);
        double et;
        if (ML) {
            et = -INFINITY;
            for (int jj = j - 1; jj <= j + 1; jj++) {
                const int jc = clampi(jj, 0, ny - 1);
                for (int ii = i - 1; ii <= i + 1; ii++) {
                    const double v = a.f.eta[clampi(ii, 0, nx - 1) + (i64)nx * jc];
                    if (v > et) et = v;
                }
            }
            const_cast<double *>(a.etatau)[c] = et;
        } else et = a.etatau[c];
        const double psi = 1.0 / (1.0 / et + _Gdt) * a.r / a.theta_dtau;
        theta[c] = (fma(P0, _Kdt, rhs) * psi + P) / (1.0 + _Kdt * psi);
        const double d3 = divV * (1.0 / 3.0);
        a.f.exx[c] = dxi - d3;
        a.f.eyy[c] = dyi - d3;
        if (RHO) a.f.fy[c] = mat_density_ratio(a.rh, a.f.phase_c + (i64)a.rh.nphase * c, !a.f.T ? 0.0 : (a.tg ? a.f.T[i + (i64)(nx + 2) * j] : a.f.T[c]), a.f.P[c]) * a.rh.gravity;
    }
    a.f.exy[i + (i64)(nx + 1) * j] = 0.5 * (spc(a.sp.vxy, j, a._dy) * (VX(i, j + 1) - VX(i, j)) + spc(a.sp.vyx, i, a._dx) * (VY(i + 1, j) - VY(i, j)));
#undef VX
#undef VY
}

// strain_increment variant (Stokes2D.jl:659-661, 680-692): ∇U and Δε from the displacements (compute_∇V!, compute_strain_rate! on U), then
// ε = Δε * _dt (compute_strain_rate_from_increment!, VelocityKernels.jl:46-57) -- overwrites the ε that k_vep_pre derived from V
__global__ __launch_bounds__(256) void k_vep_strain_inc(const VepArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ Ux = a.f.Ux, *__restrict__ Uy = a.f.Uy;
    const double _dt = 1.0 / a.dt;
#define UX(i_, j_) Ux[(i_) + (i64)(nx + 1) * (j_)]
#define UY(i_, j_) Uy[(i_) + (i64)(nx + 2) * (j_)]
    if (i < nx && j < ny) {
        const i64 c = i + (i64)nx * j;
        const double dxi = (-UX(i, j + 1) + UX(i + 1, j + 1)) * a._dx;
        const double dyi = (-UY(i + 1, j) + UY(i + 1, j + 1)) * a._dy;
        const double divU = dxi + dyi;
        a.f.divU[c] = divU;
        const double d3 = divU * (1.0 / 3.0);
        const double dexx = dxi - d3, deyy = dyi - d3;
        a.f.dexx[c] = dexx; a.f.deyy[c] = deyy;
        a.f.exx[c] = dexx * _dt; a.f.eyy[c] = deyy * _dt;
    }
    const double dexy = 0.5 * (a._dy * (UX(i, j + 1) - UX(i, j)) + a._dx * (UY(i + 1, j) - UY(i, j)));
    a.f.dexy[i + (i64)(nx + 1) * j] = dexy;
    a.f.exy[i + (i64)(nx + 1) * j] = dexy * _dt;
#undef UX
#undef UY
}
// compute_stress_increment(τ, τ_o, η, Δε, _G, dτ_r, dt) -- StressKernels.jl:18-21
// k_vep_pre<ML = true> for uniform grids and constant densities with every operand requested up front (option "fused2d_batch"): the control-flow form issues its 24 loads in five
// dependent groups (the 3 x 3 window of η compares as it loads, every `if (a.obs)` ends a basic block); same arithmetic, expression for expression.  OBS: a.obs as a constant.  TH: as in k_vep_pre.
template <bool OBS, bool TH = false>
__global__ __launch_bounds__(256) void k_vep_pre_b(const VepArgs a, double *__restrict__ theta)
{
    const int nx = a.nx, ny = a.ny;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy;
    const bool cell = i < nx && j < ny;
    const int ic = min(i, nx - 1), jc = min(j, ny - 1);
    const i64 c = ic + (i64)nx * jc;
    // velocities: Vx[i, j], Vx[i, j+1], Vx[i+1, j+1] (cells only), Vy[i, j], Vy[i+1, j], Vy[i+1, j+1] (cells only)
    const i64 qx = i + (i64)(nx + 1) * j, qy = i + (i64)(nx + 2) * j;
    const double x00 = Vx[qx], x01 = Vx[qx + (nx + 1)], x11 = Vx[qx + (nx + 1) + (i < nx ? 1 : 0)];
    const double y00 = Vy[qy], y10 = Vy[qy + 1], y11 = Vy[qy + 1 + (j < ny ? nx + 2 : 0)];
    const double Kc = a.Kc[c], Gc = a.Gc[c], P = theta[c], P0 = a.f.P0[c], Q = a.f.Q[c];
    const double S = TH ? a.src[c] : 0.0;
    double w[9];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const i64 r = (i64)nx * clampi(jc + q - 1, 0, ny - 1);
#pragma unroll
        for (int m = 0; m < 3; m++) w[3 * q + m] = a.f.eta[clampi(ic + m - 1, 0, nx - 1) + r];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (cell) {
        const double dxi = (-x01 + x11) * a._dx;
        const double dyi = (-y10 + y11) * a._dy;
        const double divV = dxi + dyi;
        if (OBS) a.f.divV[c] = divV;
        const double _Kdt = 1.0 / (Kc * a.dt), _Gdt = 1.0 / (Gc * a.dt), _dt = 1.0 / a.dt;
        const double rhs = TH ? (-divV + S) + (Q * _dt) : -divV + (Q * _dt);
        if (OBS) a.f.RP[c] = fma(-(P - P0), _Kdt, rhs);
        double et = -INFINITY;
#pragma unroll
        for (int q = 0; q < 9; q++)
            if (w[q] > et) et = w[q];
        const_cast<double *>(a.etatau)[c] = et;
        const double psi = 1.0 / (1.0 / et + _Gdt) * a.r / a.theta_dtau;
        theta[c] = (fma(P0, _Kdt, rhs) * psi + P) / (1.0 + _Kdt * psi);
        const double d3 = divV * (1.0 / 3.0);
        a.f.exx[c] = dxi - d3;
        a.f.eyy[c] = dyi - d3;
    }
    a.f.exy[qx] = 0.5 * (a._dy * (x01 - x00) + a._dx * (y10 - y00));
}

__device__ __forceinline__ double dev_stress_inc_dt(double t, double to, double eta, double de, double _G, double dtr, double dt)
{
    return dtr * fma(2.0 * eta, de, fma(-(t - to) * eta, _G, -t * dt));
}

// update_stresses_center_vertex_ps! -- vertex half.  Runs before the centre half so that the vertex averages
// see the old centre stresses (the reference's single launch races on them).
// SI: strain_increment form (StressKernels.jl:1147-1302): Δε instead of ε, _G and dτ_r = inv(θ_dτ dt + η _G + dt), plastic terms times dt
template <bool SOFT, bool SI = false, int NP = 0>
__device__ __forceinline__ void vep_vertex_at(const VepArgs &a, const int i, const int j)
{
    const int nx = a.nx, ny = a.ny, np = NP > 0 ? NP : a.rh.nphase;
    const int i0 = clampi(i - 1, 0, nx - 1), ic = clampi(i, 0, nx - 1), j0 = clampi(j - 1, 0, ny - 1), jc = clampi(j, 0, ny - 1);
#define AVC(A) (0.25 * (C2(A, i0, j0) + C2(A, ic, jc) + C2(A, i0, jc) + C2(A, ic, j0)))
    const double Pv = AVC(a.theta), exxv = SI ? AVC(a.f.dexx) : AVC(a.f.exx), eyyv = SI ? AVC(a.f.deyy) : AVC(a.f.eyy), txxv = AVC(a.f.txx), tyyv = AVC(a.f.tyy);
    const double toxxv = AVC(a.f.toxx), toyyv = AVC(a.f.toyy);
    const double EIIv = SOFT ? AVC(a.f.EII_pl) : 0.0;      // EIIv_ij = av_clamped(EII, Ic...) (StressKernels.jl:1030); only softening laws read it
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
    const double _Gdt = SI ? 1.0 / ratio_avg(a.rh.G, rv, np) : 1.0 / (ratio_avg(a.rh.G, rv, np) * a.dt);      // SI: _Gv
    const double Kv = ratio_avg(a.rh.Kb, rv, np);
    const double etav = 4.0 / (1.0 / C2(a.f.eta, i0, j0) + 1.0 / C2(a.f.eta, ic, jc) + 1.0 / C2(a.f.eta, i0, jc) + 1.0 / C2(a.f.eta, ic, j0));
    const double dtr = SI ? 1.0 / (a.theta_dtau * a.dt + etav * _Gdt + a.dt) : 1.0 / (a.theta_dtau + etav * _Gdt + 1.0);
    const double txy = a.f.txy[v];
    const double dxx = SI ? dev_stress_inc_dt(txxv, toxxv, etav, exxv, _Gdt, dtr, a.dt) : dev_stress_inc(txxv, toxxv, etav, exxv, _Gdt, dtr);
    const double dyy = SI ? dev_stress_inc_dt(tyyv, toyyv, etav, eyyv, _Gdt, dtr, a.dt) : dev_stress_inc(tyyv, toyyv, etav, eyyv, _Gdt, dtr);
    const double dxy = SI ? dev_stress_inc_dt(txy, a.f.toxy[v], etav, a.f.dexy[v], _Gdt, dtr, a.dt) : dev_stress_inc(txy, a.f.toxy[v], etav, a.f.exy[v], _Gdt, dtr);
    const double tt[3] = {txxv + dxx, tyyv + dyy, txy + dxy};
    const double tIIv = sinv2(dxx + txxv, dyy + tyyv, dxy + txy);
    double dQdt[3], dQdP, dFdP;
    plastic_grad<2, 3, NP>(a.rh, rv, tt, dQdt, dQdP, dFdP);
    const double vol = isinf(Kv) ? 0.0 : Kv * a.dt * dFdP * dQdP;
    const double F = yield_F<SOFT, NP>(a.rh, rv, Pv, tIIv, EIIv);
    if (is_pl && tIIv != 0.0 && F > 0) {
        const double l = fma(1.0 - a.rel, a.lamv[v], a.rel * (fmax(F, 0.0) / (SI ? etav * dtr * a.dt + eta_reg + vol : etav * dtr + eta_reg + vol)));
        a.lamv[v] = l;
        const double epl = l * dQdt[2];
        a.f.txy[v] = txy + (SI ? fma(-2.0 * etav * a.dt * epl, dtr, dxy) : fma(-2.0 * etav * epl, dtr, dxy));
        if (a.obs) a.f.eplxy[v] = epl;
    } else {
        a.f.txy[v] = txy + dxy;
        if (a.obs) a.f.eplxy[v] = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_vep_vertex(const VepArgs a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / (a.nx + 1), i = t - j * (a.nx + 1);
    if (j > a.ny) return;
    if (a.si) { if (a.soft) vep_vertex_at<true, true>(a, i, j); else vep_vertex_at<false, true>(a, i, j); }
    else if (a.soft) vep_vertex_at<true>(a, i, j);
    else vep_vertex_at<false>(a, i, j);
}

// operands of the centre half, loaded up front: in the merged launch they are requested BEFORE the vertex half stores anything (the compiler cannot move
// loads above stores through unrelated pointers), so that the two halves' memory round trips overlap
struct CentreOps { double e, exyc, exx, eyy, txx, tyy, txyc, toxx, toyy, toxyc, theta, lam, EII, dexx, deyy, dexyc; };
template <bool SOFT, bool SI>
__device__ __forceinline__ CentreOps vep_centre_load(const VepArgs &a, const int i, const int j)
{
    const int nx = a.nx;
    const i64 c = i + (i64)nx * j;
    CentreOps o;
    o.e = a.f.eta[c];
    o.exyc = (V2(a.f.exy, i, j) + V2(a.f.exy, i + 1, j) + V2(a.f.exy, i, j + 1) + V2(a.f.exy, i + 1, j + 1)) / 4;
    o.exx = a.f.exx[c]; o.eyy = a.f.eyy[c];
    o.txx = a.f.txx[c]; o.tyy = a.f.tyy[c]; o.txyc = a.f.txy_c[c];
    o.toxx = a.f.toxx[c]; o.toyy = a.f.toyy[c]; o.toxyc = a.f.toxy_c[c];
    o.theta = a.theta[c]; o.lam = a.lam[c];
    o.EII = SOFT ? a.f.EII_pl[c] : 0.0;
    if (SI) {      // Δεij = (Δε.xx, Δε.yy, av_shear(Δε.xy)) -- cache_tensors, StressUpdate.jl:226-246
        o.dexyc = (V2(a.f.dexy, i, j) + V2(a.f.dexy, i + 1, j) + V2(a.f.dexy, i, j + 1) + V2(a.f.dexy, i + 1, j + 1)) / 4;
        o.dexx = a.f.dexx[c]; o.deyy = a.f.deyy[c];
    } else o.dexyc = o.dexx = o.deyy = 0.0;
    return o;
}

// update_stresses_center_vertex_ps! -- centre half (+ Pr_c, τII, η_vep)
template <bool SOFT, bool SI = false, int NP = 0>
__device__ __forceinline__ void vep_centre_at(const VepArgs &a, const int i, const int j, const CentreOps &o)
{
    const int nx = a.nx, np = NP > 0 ? NP : a.rh.nphase;
    const i64 c = i + (i64)nx * j;
    double *__restrict__ txx_o = a.txx_out ? a.txx_out : a.f.txx, *__restrict__ tyy_o = a.tyy_out ? a.tyy_out : a.f.tyy;
    double rcv[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
        for (int q = 0; q < NP; q++) rcv[q] = a.f.phase_c[(i64)NP * c + q];
    }
    const double *rc = NP > 0 ? rcv : a.f.phase_c + (i64)np * c;
    const double _Gdt = SI ? 1.0 / ratio_avg(a.rh.G, rc, np) : 1.0 / (ratio_avg(a.rh.G, rc, np) * a.dt);
    bool is_pl; double eta_reg;
    plastic_params<NP>(a.rh, rc, is_pl, eta_reg);
    const double K = ratio_avg(a.rh.Kb, rc, np);
    const double e = o.e;
    const double dtr = SI ? 1.0 / (a.theta_dtau * a.dt + e * _Gdt + a.dt) : 1.0 / (a.theta_dtau + e * _Gdt + 1.0);
    const double eij[3] = {o.exx, o.eyy, o.exyc};
    double tij[3] = {o.txx, o.tyy, o.txyc};
    const double toij[3] = {o.toxx, o.toyy, o.toxyc};
    double d[3];
    if (SI) {
        const double deij[3] = {o.dexx, o.deyy, o.dexyc};
#pragma unroll
        for (int q = 0; q < 3; q++) d[q] = dev_stress_inc_dt(tij[q], toij[q], e, deij[q], _Gdt, dtr, a.dt);
    } else {
#pragma unroll
        for (int q = 0; q < 3; q++) d[q] = dev_stress_inc(tij[q], toij[q], e, eij[q], _Gdt, dtr);
    }
    double tII = sinv2(d[0] + tij[0], d[1] + tij[1], d[2] + tij[2]);
    const double tt[3] = {tij[0] + d[0], tij[1] + d[1], tij[2] + d[2]};
    double dQdt[3], dQdP, dFdP;
    plastic_grad<2, 3, NP>(a.rh, rc, tt, dQdt, dQdP, dFdP);
    const double vol = isinf(K) ? 0.0 : K * a.dt * dFdP * dQdP;
    const double Pr = o.theta;
    const double F = yield_F<SOFT, NP>(a.rh, rc, Pr, tII, o.EII);
    double l = o.lam;
    if (is_pl && tII != 0.0 && F > 0) {
        l = fma(1.0 - a.rel, l, a.rel * (fmax(F, 0.0) / (SI ? e * dtr * a.dt + eta_reg + vol : e * dtr + eta_reg + vol)));
        a.lam[c] = l;
        double epl[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            epl[q] = l * dQdt[q];
            d[q] = SI ? fma(-2.0 * e * a.dt * epl[q], dtr, d[q]) : fma(-2.0 * e * epl[q], dtr, d[q]);
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
__global__ __launch_bounds__(256) void k_vep_centre(const VepArgs a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / a.nx, i = t - j * a.nx;
    if (j >= a.ny) return;
    if (a.si) { if (a.soft) vep_centre_at<true, true>(a, i, j, vep_centre_load<true, true>(a, i, j)); else vep_centre_at<false, true>(a, i, j, vep_centre_load<false, true>(a, i, j)); }
    else if (a.soft) vep_centre_at<true>(a, i, j, vep_centre_load<true, false>(a, i, j));
    else vep_centre_at<false>(a, i, j, vep_centre_load<false, false>(a, i, j));
}
// both halves in one launch: the vertex half averages the OLD centre stresses, so the centre half must write τxx, τyy elsewhere
// (a.txx_out / a.tyy_out; the caller then swaps the pointers)
template <bool SOFT, bool SI = false, int NP = 0>
__global__ __launch_bounds__(256) void k_vep_stress2d(const VepArgs a)
{
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (a.nx + 1), i = t - j * (a.nx + 1);
    if (j > a.ny) return;
    const bool cell = i < a.nx && j < a.ny;
    CentreOps o = {};
    if (cell) o = vep_centre_load<SOFT, SI>(a, i, j);          // before the vertex half's stores
    vep_vertex_at<SOFT, SI, NP>(a, i, j);
    if (cell) vep_centre_at<SOFT, SI, NP>(a, i, j, o);
}

// compute_τ_nonlinear! 2D: single phase (StressKernels.jl:266-307) / phases at the cell centres (:310-351) with
// _compute_τ_nonlinear! (rheology/StressUpdate.jl:2-57).  Centre-only; τ_old.xy and ε_pl.xy are the vertex arrays
// addressed with the centre's [i,j], as the reference's caller passes them (Stokes2D.jl:442-458).
template <bool MULTI>
__global__ __launch_bounds__(256) void k_tau_nonlinear2d(const VepArgs a, double *__restrict__ theta_out)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const i64 c = i + (i64)nx * j;
    const double one = 1.0;
    const double *r = MULTI ? a.f.phase_c + (i64)np * c : &one;
    const int n = MULTI ? np : 1;
    const double e = a.f.eta[c], dt = a.dt;
    const double _Gdt = 1.0 / ((MULTI ? ratio_avg(a.rh.G, r, n) : a.rh.G[0]) * dt);
    const double dtr = dev_dtau_r(a.theta_dtau, e, _Gdt);
    bool is_pl = false;
    double C = 0.0, sinphi = 0.0, cosphi = 0.0, sinpsi = 0.0, eta_reg = 0.0;
    for (int q = 0; q < n; q++) {
        if (r[q] == 0.0 || !a.rh.is_pl[q]) continue;
        is_pl = true;
        const double EII = a.soft ? a.f.EII_pl[c] : 0.0;         // soften_cohesion / soften_friction_angle at EII[I...] (StressUpdate.jl:305-381)
        double sp, cp;
        mat_friction(a.rh, q, EII, sp, cp);
        C += mat_cohesion(a.rh, q, EII) * r[q]; sinphi += sp * r[q]; cosphi += cp * r[q];
        sinpsi += a.rh.sinpsi[q] * r[q]; eta_reg += a.rh.eta_vp[q] * r[q];
    }
    const double K = MULTI ? ratio_avg(a.rh.Kb, r, n) : a.rh.Kb[0];
    const double volume = isinf(K) ? 0.0 : K * dt * sinphi * sinpsi;
    const double eij[3] = {a.f.exx[c], a.f.eyy[c], (V2(a.f.exy, i, j) + V2(a.f.exy, i + 1, j) + V2(a.f.exy, i, j + 1) + V2(a.f.exy, i + 1, j + 1)) / 4};
    const double tij[3] = {a.f.txx[c], a.f.tyy[c], a.f.txy_c[c]};
    const double toij[3] = {a.f.toxx[c], a.f.toyy[c], V2(a.f.toxy, i, j)};
    const double P = a.f.P[c];
    double d[3], ldq[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 3; q++) d[q] = dev_stress_inc(tij[q], toij[q], e, eij[q], _Gdt, dtr);
    const double tII_trial = sinv2(tij[0] + d[0], tij[1] + d[1], tij[2] + d[2]);
    const double ty = fmax(C * cosphi + P * sinphi, 0.0);
    double l = a.lam[c];
    if (is_pl && tII_trial > ty) {
        const double F = tII_trial - ty;
        l = 0.5 * l + (1 - 0.5) * (F > 0.0 ? 1.0 : 0.0) * F * (1.0 / (e * dtr + eta_reg + volume));
        const double l_tII = l * 0.5 * (1.0 / tII_trial);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            ldq[q] = (tij[q] + d[q]) * l_tII;
            d[q] = fma(-dtr * 2.0, e * ldq[q], d[q]);
        }
        a.lam[c] = l;
    }
    a.f.eplxx[c] = isinf(ldq[0]) ? 0.0 : ldq[0];
    a.f.eplyy[c] = isinf(ldq[1]) ? 0.0 : ldq[1];
    V2(a.f.eplxy, i, j) = isinf(ldq[2]) ? 0.0 : ldq[2];
    a.f.txx[c] = tij[0] + d[0]; a.f.tyy[c] = tij[1] + d[1]; a.f.txy_c[c] = tij[2] + d[2];
    const double tII = sinv2(tij[0] + d[0], tij[1] + d[1], tij[2] + d[2]);
    a.f.tII[c] = tII;
    a.f.eta_vep[c] = tII * 0.5 * (1.0 / sinv2(eij[0], eij[1], eij[2]));
    theta_out[c] = P + (isinf(K) ? 0.0 : K * dt * l * sinpsi);
}

// center2vertex! 2D (Interpolations.jl:101-114): pass 0 inner vertices, pass 1 the x-edge rows, pass 2 the y-edge columns; pass 3 = the three at once: after
// them every edge / corner vertex is a copy of the inner vertex its indices clamp to, so each thread evaluates that one
__global__ __launch_bounds__(256) void k_center2vertex2d(double *__restrict__ v, const double *__restrict__ cc, int nx, int ny, int pass)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (pass == 3) {
        const int j = t / (nx + 1), i = t - j * (nx + 1);
        if (j > ny) return;
        const int ii = clampi(i, 1, nx - 1), jj = clampi(j, 1, ny - 1);
        v[i + (i64)(nx + 1) * j] = 0.25 * (cc[(ii - 1) + (i64)nx * (jj - 1)] + cc[ii + (i64)nx * (jj - 1)] + cc[(ii - 1) + (i64)nx * jj] + cc[ii + (i64)nx * jj]);
    } else if (pass == 0) {
        const int j = t / (nx + 1), i = t - j * (nx + 1);
        if (j > ny || i < 1 || i >= nx || j < 1 || j >= ny) return;
        v[i + (i64)(nx + 1) * j] = 0.25 * (cc[(i - 1) + (i64)nx * (j - 1)] + cc[i + (i64)nx * (j - 1)] + cc[(i - 1) + (i64)nx * j] + cc[i + (i64)nx * j]);
    } else if (pass == 1) {
        if (t > ny) return;
        v[0 + (i64)(nx + 1) * t] = v[1 + (i64)(nx + 1) * t];
        v[nx + (i64)(nx + 1) * t] = v[nx - 1 + (i64)(nx + 1) * t];
    } else {
        if (t > nx) return;
        v[t] = v[t + (i64)(nx + 1)];
        v[t + (i64)(nx + 1) * ny] = v[t + (i64)(nx + 1) * (ny - 1)];
    }
}

__device__ __forceinline__ double phase_viscosity(const jrx_rheology &rh, const double *r)
{   // compute_phase_viscosity, rheology/Viscosity.jl:605-625 (LinearViscous elements)
    for (int q = 0; q < rh.nphase; q++)
        if (r[q] > 0.999) return rh.eta[q];
    double s = 0.0;
    for (int q = 0; q < rh.nphase; q++)
        if (r[q] != 0.0) s += (1.0 / rh.eta[q]) * r[q];
    return 1.0 / s;
}
// compute_viscosity_kernel! at a centre / a vertex for creep laws that read fields (rheology/Viscosity.jl:382-418): the invariant of @stress_center /
// @strain_center, args at the cell (T at I .+ 1 of the ghosted thermal.T, local_viscosity_args :513-523); at a vertex (xx_v, yy_v, xy) -- the PT solvers
// never write xx_v, yy_v: zero -- and args averaged over the clamped surrounding centres, T over its 2 x 2 nodes (local_viscosity_args_vertex :528-552)
__device__ __forceinline__ double vep_visc_fields_centre(const VepArgs &a, const i64 t)
{
    const int nx = a.nx, j = (int)(t / nx), i = (int)(t - (i64)j * nx);
    const double AII = a.vtau ? mat_visc_invariant2(a.f.txx[t], a.f.tyy[t], a.f.txy_c[t]) : mat_visc_invariant2(a.f.exx[t], a.f.eyy[t], a.f.exy_c[t]);
    const double T = !a.f.T ? 0.0 : (a.tg ? a.f.T[(i + 1) + (i64)(nx + 2) * (j + 1)] : a.f.T[t]);
    return mat_phase_viscosity(a.rh, a.f.phase_c + (i64)a.rh.nphase * t, AII, T, a.f.P[t], a.vtau);
}
__device__ __forceinline__ double vep_visc_fields_vertex(const VepArgs &a, const i64 t)
{
    const int nx = a.nx, ny = a.ny, j = (int)(t / (nx + 1)), i = (int)(t - (i64)j * (nx + 1));
    const int il = max(i - 1, 0), ir = min(i, nx - 1), jb = max(j - 1, 0), jt = min(j, ny - 1);
    const double AII = mat_visc_invariant2(0.0, 0.0, a.vtau ? a.f.txy[t] : a.f.exy[t]);
    const double P = 0.25 * (a.f.P[il + (i64)nx * jb] + a.f.P[ir + (i64)nx * jb] + a.f.P[il + (i64)nx * jt] + a.f.P[ir + (i64)nx * jt]);
    double T = 0.0;
    if (a.f.T && a.tg) {
        const double *q = a.f.T + i + (i64)(nx + 2) * j;
        T = 0.25 * (q[0] + q[1] + q[nx + 2] + q[nx + 3]);
    } else if (a.f.T) T = 0.25 * (a.f.T[il + (i64)nx * jb] + a.f.T[ir + (i64)nx * jb] + a.f.T[il + (i64)nx * jt] + a.f.T[ir + (i64)nx * jt]);
    return mat_phase_viscosity(a.rh, a.f.phase_v + (i64)a.rh.nphase * t, AII, T, P, a.vtau);
}
__device__ __forceinline__ void vep_visc_at(const VepArgs &a, const i64 t)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    if (a.vfields) {
        if (t < (i64)nx * ny) {
            const double e = vep_visc_fields_centre(a, t) * a.nu + a.f.eta[t] * (1.0 - a.nu);
            a.f.eta[t] = fmin(fmax(e, a.cut_lo), a.cut_hi);
        }
        if (a.f.eta_v && t < (i64)(nx + 1) * (ny + 1)) {
            const double e = vep_visc_fields_vertex(a, t) * a.nu + a.f.eta_v[t] * (1.0 - a.nu);
            a.f.eta_v[t] = fmin(fmax(e, a.cut_lo), a.cut_hi);
        }
        return;
    }
    if (t < (i64)nx * ny) {
        double e = a.eta_lin_c ? a.eta_lin_c[t] : phase_viscosity(a.rh, a.f.phase_c + np * t);
        e = e * a.nu + a.f.eta[t] * (1.0 - a.nu);
        a.f.eta[t] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
    if (a.f.eta_v && t < (i64)(nx + 1) * (ny + 1)) {
        double e = a.eta_lin_v ? a.eta_lin_v[t] : phase_viscosity(a.rh, a.f.phase_v + np * t);
        e = e * a.nu + a.f.eta_v[t] * (1.0 - a.nu);
        a.f.eta_v[t] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
}
__global__ __launch_bounds__(256) void k_vep_visc(const VepArgs a) { vep_visc_at(a, (i64)blockIdx.x * blockDim.x + threadIdx.x); }
// compute_viscosity! and compute_V! in one launch: the velocity update reads ητ (already taken from the previous η), P, τ, ρg, never η
template <bool BCF>
__global__ __launch_bounds__(256) void k_vep_visc_velocity(const VepArgs a, const Args2 b)
{
    const i64 t = (i64)xcd_slab_block() * blockDim.x + threadIdx.x;
    vep_visc_at(a, t);
    const int j = (int)(t / b.nx), i = (int)(t - (i64)j * b.nx);
    if (j < b.ny) velocity2d_cell<false, BCF>(b, i, j);
}

// k_vep_visc_velocity for laws whose η reads no field (the phase average is precomputed), uniform grids and no free surface, with every operand requested up front (option
// "fused2d_batch").  The general kernel carries the field-reading creep laws, the non-uniform spacings and the free-surface correction as run-time branches: 3,200 ISA lines, 68
// branches, its 48 loads in ~20 dependent groups.  Same arithmetic on the path it takes for these inputs, expression for expression.
template <bool BCF>
__global__ __launch_bounds__(256) void k_vep_visc_velocity_b(const VepArgs a, const Args2 b)
{
    const i64 t = (i64)xcd_slab_block() * blockDim.x + threadIdx.x;
    const int nx = b.nx, ny = b.ny;
    const i64 nc = (i64)nx * ny, nv = (i64)(nx + 1) * (ny + 1);
    const bool cell = t < nc, vert = a.f.eta_v != nullptr && t < nv;
    const i64 c = cell ? t : 0, tv = t < nv ? t : 0;
    const int j = (int)(c / nx), i = (int)(c - (i64)j * nx);
    const i64 cx = c + (i < nx - 1 ? 1 : 0), cy = c + (j < ny - 1 ? nx : 0);
    const double *__restrict__ P = b.f.P, *__restrict__ txy = b.f.txy, *__restrict__ et = b.etatau;
    const i64 qx = (i + 1) + (i64)(nx + 1) * (j + 1), qy = (i + 1) + (i64)(nx + 2) * (j + 1);
    // ---- every operand
    const double el = a.eta_lin_c[c], eo = a.f.eta[c];
    double elv = 0.0, eov = 0.0;
    if (a.f.eta_v) { elv = a.eta_lin_v[tv]; eov = a.f.eta_v[tv]; }
    const double P0 = P[c], Px = P[cx], Py = P[cy], X0 = b.f.txx[c], X1 = b.f.txx[cx], Y0 = b.f.tyy[c], Y1 = b.f.tyy[cy];
    const double S10 = txy[(i + 1) + (i64)(nx + 1) * j], S11 = txy[(i + 1) + (i64)(nx + 1) * (j + 1)], S01 = txy[i + (i64)(nx + 1) * (j + 1)];
    const double fx0 = b.f.fx[c], fx1 = b.f.fx[cx], fy0 = b.f.fy[c], fy1 = b.f.fy[cy];
    const double E0 = et[c], Ex = et[cx], Ey = et[cy];
    const double vx0 = b.f.Vx[qx], vy0 = b.f.Vy[qy];
    __builtin_amdgcn_sched_barrier(0);
    // ---- compute_viscosity! (vep_visc_at, laws without fields)
    if (cell) {
        double e = el;
        e = e * a.nu + eo * (1.0 - a.nu);
        a.f.eta[c] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
    if (vert) {
        double e = elv;
        e = e * a.nu + eov * (1.0 - a.nu);
        a.f.eta_v[tv] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
    if (!cell) return;
    // ---- compute_V! (velocity2d_cell<false, BCF>, uniform spacing, fs_dt = 0)
    const double edt = b.eta_dtau, _dx = b._dx, _dy = b._dy;
    if (i < nx - 1) {
        const double dP = (-P0 + Px) * _dx, dT = (-X0 + X1) * _dx;
        const double dS = (-S10 + S11) * _dy, av = (fx0 + fx1) * 0.5;
        const double v = vx0 + (-dP + dT + dS - av) * edt / ((E0 + Ex) * 0.5);
        b.f.Vx[qx] = v;
        if (BCF) {      // Vx ghost rows j = 0 (bot) and j = ny+1 (top)
            if (j == 0) { if (b.fs & JRX_FACE_BOT) b.f.Vx[qx - (nx + 1)] = v; else if (b.ns & JRX_FACE_BOT) b.f.Vx[qx - (nx + 1)] = -v; }
            if (j == ny - 1) { if (b.fs & JRX_FACE_TOP) b.f.Vx[qx + (nx + 1)] = v; else if (b.ns & JRX_FACE_TOP) b.f.Vx[qx + (nx + 1)] = -v; }
        }
    }
    if (j < ny - 1) {
        const double dP = (-P0 + Py) * _dy, dT = (-Y0 + Y1) * _dy;
        const double dS = (-S01 + S11) * _dx, av = (fy0 + fy1) * 0.5;
        const double rhs = -dP + dT + dS - av;
        const double v = vy0 + rhs * edt / ((E0 + Ey) * 0.5);
        b.f.Vy[qy] = v;
        if (BCF) {      // Vy ghost columns i = 0 (left) and i = nx+1 (right)
            if (i == 0) { if (b.fs & JRX_FACE_LEFT) b.f.Vy[qy - 1] = v; else if (b.ns & JRX_FACE_LEFT) b.f.Vy[qy - 1] = -v; }
            if (i == nx - 1) { if (b.fs & JRX_FACE_RIGHT) b.f.Vy[qy + 1] = v; else if (b.ns & JRX_FACE_RIGHT) b.f.Vy[qy + 1] = -v; }
        }
    }
}

// rho: also compute_ρg!(ρg, phase_ratios, rheology, args) (Stokes2D.jl:646)
// src: args.ΔT is given -- the thermal source of compute_P!, α_c * (ΔT * _dt) with α_c = fn_ratio(get_thermal_expansion, ...) and ΔT at the cell's own [i, j] (PressureKernels.jl:147-149,201)
__global__ __launch_bounds__(256) void k_phase_avg(double *__restrict__ Kc, double *__restrict__ Gc, const VepArgs a, const bool rho, double *__restrict__ elc = nullptr,
                                                   double *__restrict__ elv = nullptr, double *__restrict__ src = nullptr)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (elv && t < (i64)(a.nx + 1) * (a.ny + 1)) elv[t] = phase_viscosity(a.rh, a.f.phase_v + a.rh.nphase * t);
    if (t >= (i64)a.nx * a.ny) return;
    if (elc) elc[t] = phase_viscosity(a.rh, a.f.phase_c + a.rh.nphase * t);
    Kc[t] = ratio_avg(a.rh.Kb, a.f.phase_c + a.rh.nphase * t, a.rh.nphase);
    Gc[t] = ratio_avg(a.rh.G, a.f.phase_c + a.rh.nphase * t, a.rh.nphase);
    if (rho) a.f.fy[t] = mat_density_ratio(a.rh, a.f.phase_c + a.rh.nphase * t, !a.f.T ? 0.0 : (a.tg ? a.f.T[(t % a.nx) + (i64)(a.nx + 2) * (t / a.nx)] : a.f.T[t]), a.f.P[t]) * a.rh.gravity;
    if (src) {
        const double dT = a.dtg ? a.f.dT[(t % a.nx) + (i64)(a.nx + 2) * (t / a.nx)] : a.f.dT[t], _dt = 1.0 / a.dt;
        src[t] = mat_thermal_expansion_ratio(a.rh, a.f.phase_c + a.rh.nphase * t) * (dT * _dt);
    }
}

// Single-phase driver (Stokes2D.jl:345-557): compute_ρg!/update_ρg!(ρg[2], rheology, args) and compute_viscosity!/compute_viscosity_τII!
// (Viscosity.jl:142-167) for creep laws without strain-rate dependence: η <- clamp((1 - ν) η + ν η_creep(T, P), cutoff).
// args.T: cell-centred (nx, ny), or -- tg -- thermal.T (nx+2, ny+2) indexed as the reference does: density at [i, j]
// (getindex_NamedTuple(args, I...), BuoyancyForces.jl:17), viscosity at [i+1, j+1] (local_viscosity_args, Viscosity.jl:513-523).
// A power-law creep takes its invariant from @strain(stokes) = (ε.xx, ε.yy, ε.xy[i, j] -- the vertex array at the cell's index) in both forms, as
// _compute_viscosity!(stokes, ν, args, rheology, cutoff, fn_viscosity) does (Viscosity.jl:136-167); a.vtau: fn_viscosity is compute_viscosity_τII.
__global__ __launch_bounds__(256) void k_single_material(const VepArgs a, const double nu, const bool rho, const bool visc, const bool tg)
{
    const int nx = a.nx, ny = a.ny;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const i64 c = i + (i64)nx * j;
    const double P = a.f.P[c];
    if (rho) {
        const double T = !a.f.T ? 0.0 : (tg ? a.f.T[i + (i64)(nx + 2) * j] : a.f.T[c]);
        a.f.fy[c] = mat_density(a.rh, 0, T, P) * a.rh.gravity;
    }
    if (visc) {
        const double T = !a.f.T ? 0.0 : (tg ? a.f.T[(i + 1) + (i64)(nx + 2) * (j + 1)] : a.f.T[c]);
        const double AII = a.rh.visc_kind[0] == 2 ? mat_visc_invariant2(a.f.exx[c], a.f.eyy[c], a.f.exy[i + (i64)(nx + 1) * j]) : 0.0;
        const double e = (1 - nu) * a.f.eta[c] + nu * mat_viscosity(a.rh, 0, AII, T, P, a.vtau);
        a.f.eta[c] = fmin(fmax(e, a.cut_lo), a.cut_hi);
    }
}
__global__ __launch_bounds__(256) void k_fill2(double *__restrict__ A, double va, double *__restrict__ B, double vb, i64 n)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { A[t] = va; B[t] = vb; }
}

__global__ __launch_bounds__(256) void k_tensor_invariant2d(double *__restrict__ II, const double *__restrict__ xx, const double *__restrict__ yy,
                                                           const double *__restrict__ xy, int nx, int ny)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    II[t] = sinv_stag(xx[t], yy[t], V2(xy, i, j), V2(xy, i + 1, j), V2(xy, i, j + 1), V2(xy, i + 1, j + 1));
}

__global__ __launch_bounds__(256) void k_axpy_dt(double *__restrict__ y, const double *__restrict__ x, double dt, i64 n)
{
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] += dt * x[t];
}

// the epilogue operators alone: mode 0 shear2center_kernel! (Interpolations.jl:306-311), 1 accumulate_tensor_kernel!
// (StressKernels.jl:379-392), 2 compute_vorticity! (stress_rotation_particles.jl:17-29; over the vertices)
__global__ __launch_bounds__(256) void k_epilogue_op2d(int mode, double *__restrict__ out, const double *A, const double *B, const double *Cv, double s1,
                                                       double s2, int nx, int ny)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == 2) {
        const int j = t / (nx + 1), i = t - j * (nx + 1);
        if (j > ny) return;
        // A = Vx (nx+1, ny+2), B = Vy (nx+2, ny+1); s1 = _dx, s2 = _dy
        V2(out, i, j) = 0.5 * ((-B[i + (i64)(nx + 2) * j] + B[(i + 1) + (i64)(nx + 2) * j]) * s1 - (-A[i + (i64)(nx + 1) * j] + A[i + (i64)(nx + 1) * (j + 1)]) * s2);
        return;
    }
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const i64 c = i + (i64)nx * j;
    if (mode == 0) out[c] = 0.25 * (V2(Cv, i, j) + V2(Cv, i + 1, j) + V2(Cv, i, j + 1) + V2(Cv, i + 1, j + 1));
    else out[c] += sinv_stag(A[c], B[c], V2(Cv, i, j), V2(Cv, i + 1, j), V2(Cv, i, j + 1), V2(Cv, i + 1, j + 1)) * s1;
}

// post-loop epilogue: compute_vorticity!, shear2center! x3, accumulate_tensor!, accumulate_vol! (Stokes2D.jl:831-843)
__global__ __launch_bounds__(256) void k_vep_epilogue(const VepArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    if (a.f.omega_xy)
        V2(a.f.omega_xy, i, j) = 0.5 * ((-a.f.Vy[i + (i64)(nx + 2) * j] + a.f.Vy[(i + 1) + (i64)(nx + 2) * j]) * spc(a.sp.vyx, i, a._dx) -
                                        (-a.f.Vx[i + (i64)(nx + 1) * j] + a.f.Vx[i + (i64)(nx + 1) * (j + 1)]) * spc(a.sp.vxy, j, a._dy));
    if (i < nx && j < ny) {
        const i64 c = i + (i64)nx * j;
#define S2C(V) (0.25 * (V2(V, i, j) + V2(V, i + 1, j) + V2(V, i, j + 1) + V2(V, i + 1, j + 1)))
        if (a.f.exy_c) a.f.exy_c[c] = S2C(a.f.exy);
        if (a.f.eplxy_c) a.f.eplxy_c[c] = S2C(a.f.eplxy);
        if (a.f.dexy_c && a.f.dexy) a.f.dexy_c[c] = S2C(a.f.dexy);
#undef S2C
        a.f.EII_pl[c] += sinv_stag(a.f.eplxx[c], a.f.eplyy[c], V2(a.f.eplxy, i, j), V2(a.f.eplxy, i + 1, j), V2(a.f.eplxy, i, j + 1),
                                   V2(a.f.eplxy, i + 1, j + 1)) * a.dt;
        a.f.EVol_pl[c] += a.dt * a.f.evol_pl[c];
    }
}
#undef C2
#undef V2

jrx_status check_vep(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !rh || !p) return jrx_fail(h, JRX_ERR_ARG, "null VEP argument");
    JRX_TRY(jrx_check_device(h));
    if (p->nx < 3 || p->ny < 3) return jrx_fail(h, JRX_ERR_ARG, "2D Stokes needs at least 3 cells per dimension");
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
    const void *req[] = {f->P, f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Ux, f->Uy, f->exx, f->eyy, f->exy, f->eplxx, f->eplyy, f->eplxy, f->eplxy_c,
                         f->txx, f->tyy, f->txy, f->txy_c, f->tII, f->toxx, f->toyy, f->toxy, f->toxy_c, f->eta, f->eta_vep, f->EII_pl, f->evol_pl,
                         f->EVol_pl, f->fx, f->fy, f->RP, f->Rx, f->Ry, f->phase_c, f->phase_v};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "a required VEP field pointer is NULL");
    if (p->strain_increment && (!f->dexx || !f->deyy || !f->dexy || !f->divU))
        return jrx_fail(h, JRX_ERR_ARG, "strain_increment: the Δε (xx, yy, xy) and ∇U arrays are required");
    if (!jrx2d_spacing_ok(p->inv_spacing)) return jrx_fail(h, JRX_ERR_ARG, "non-uniform grid: all six inverse-spacing arrays are required");
    if (p->inv_spacing[0] && p->strain_increment)
        return jrx_fail(h, JRX_ERR_UNSUPPORTED, "strain_increment on a non-uniform grid is not built (the reference's own kernel indexes _di.center beyond its extent there)");
    return JRX_OK;
}

VepArgs make_vep(const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p)
{
    VepArgs a;
    memset(&a, 0, sizeof(a));
    a.f = *f; a.rh = *rh;
    a._dx = p->_dx; a._dy = p->_dy; a.dt = p->dt; a.r = p->r; a.theta_dtau = p->theta_dtau; a.rel = p->lambda_relaxation;
    a.nu = p->viscosity_relaxation; a.cut_lo = p->cutoff_lo; a.cut_hi = p->cutoff_hi;
    a.nx = (int)p->nx; a.ny = (int)p->ny;
    a.soft = mat_has_softening(rh);
    a.si = p->strain_increment != 0;
    a.tg = p->T_ghosted != 0;
    a.dtg = p->dT_ghosted != 0;
    a.vfields = mat_viscosity_reads_fields(rh); a.vtau = true;
    a.obs = true;
    a.sp = Sp2{p->inv_spacing[0], p->inv_spacing[1], p->inv_spacing[2], p->inv_spacing[3], p->inv_spacing[4], p->inv_spacing[5]};
    return a;
}

// args.ΔT with args.melt_fraction: the reference then takes α(ϕ) from GeoParams (PressureKernels.jl:154-176) in a form nothing under it states
jrx_status check_vep_thermal(jrx_handle *h, const jrx_vep2d_fields *f)
{
    if (f->dT && f->melt_fraction)
        return jrx_fail(h, JRX_ERR_ARG, "compute_P!: args.melt_fraction together with args.ΔT (the melt-dependent thermal expansion α(ϕ)) is not built");
    return JRX_OK;
}

// the pre kernel of the multiphase driver.  ml: compute_maxloc! folded in (ranks with neighbours exchange ητ instead); rho: update_ρg!; batch: the form that requests every operand
// up front (ml, no rho, uniform grids); a.src != nullptr: the thermal forms (args.ΔT).  Without it the instantiations are those of the isothermal driver.
void launch_vep_pre(hipStream_t s, unsigned gv, const VepArgs &a, double *theta, bool ml, bool rho, bool batch)
{
    const std::true_type yes{};
    const std::false_type no{};
    auto go = [&](auto TH_) {
        constexpr bool TH = decltype(TH_)::value;
        if (!ml && rho) hipLaunchKernelGGL((k_vep_pre<false, true, TH>), dim3(gv), dim3(256), 0, s, a, theta);
        else if (!ml) hipLaunchKernelGGL((k_vep_pre<false, false, TH>), dim3(gv), dim3(256), 0, s, a, theta);
        else if (rho) hipLaunchKernelGGL((k_vep_pre<true, true, TH>), dim3(gv), dim3(256), 0, s, a, theta);
        else if (batch && a.obs) hipLaunchKernelGGL((k_vep_pre_b<true, TH>), dim3(gv), dim3(256), 0, s, a, theta);
        else if (batch) hipLaunchKernelGGL((k_vep_pre_b<false, TH>), dim3(gv), dim3(256), 0, s, a, theta);
        else hipLaunchKernelGGL((k_vep_pre<true, false, TH>), dim3(gv), dim3(256), 0, s, a, theta);      // compute_maxloc! folded in
    };
    if (a.src) go(yes); else go(no);
}

// compute_viscosity! (tau = false: the invariant from the strain rate) / update_viscosity_τII! (tau = true: from the stress) as entry points of their own
jrx_status vep2_viscosity(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu, bool tau)
{
    JRX_TRY(check_vep(h, f, rh, p));
    VepArgs a = make_vep(f, rh, p);
    a.nu = nu; a.vtau = tau;
    hipLaunchKernelGGL(k_vep_visc, dim3((unsigned)(((p->nx + 1) * (p->ny + 1) + 255) / 256)), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

// the velocity / residual kernels of the visco-elastic path work on this view (P = stokes.P = Pr_c, τxy at vertices)
jrx_stokes2d_fields view2d(const jrx_vep2d_fields *f)
{
    jrx_stokes2d_fields g;
    memset(&g, 0, sizeof(g));
    g.P = f->P; g.P0 = f->P0; g.divV = f->divV; g.Q = f->Q; g.Vx = f->Vx; g.Vy = f->Vy; g.Ux = f->Ux; g.Uy = f->Uy;
    g.txx = f->txx; g.tyy = f->tyy; g.txy = f->txy; g.exx = f->exx; g.eyy = f->eyy; g.exy = f->exy; g.eta = f->eta;
    g.fx = f->fx; g.fy = f->fy; g.RP = f->RP; g.Rx = f->Rx; g.Ry = f->Ry;
    return g;
}

// update_stresses_center_vertex_ps!: vertex and centre halves in one launch.  Softening laws and the strain_increment form take the general kernel, otherwise the phase
// count is a constant up to four (option vep3_np_const; more phases: 0, the run-time count)
void launch_vep_stress2d(jrx_handle *h, hipStream_t s, unsigned gv, const VepArgs &a)
{
    const std::true_type yes{};
    const std::false_type no{};
    const std::integral_constant<int, 0> np0{};
    auto go = [&](auto SOFT, auto SI, auto NP) { hipLaunchKernelGGL((k_vep_stress2d<SOFT(), SI(), NP()>), dim3(gv), dim3(256), 0, s, a); };
    if (a.si && a.soft) go(yes, yes, np0);
    else if (a.si) go(no, yes, np0);
    else if (a.soft) go(yes, no, np0);
    else dispatch_const<0, 1, 2, 3, 4>(h->vep3_np_const && a.rh.nphase <= 4 ? a.rh.nphase : 0, [&](auto NP) { go(no, no, NP); });
}

// What one PT iteration of the multiphase solve loop works on: the arguments of the VEP kernels (a), of the velocity kernels (b) and the view the norms take (g), which all
// name the current (τxx, τyy).  The stress kernel writes the other set (a.txx_out, a.tyy_out) and adopting its output is a swap, so the captured graphs of an even number of
// iterations, which run on a copy, end where they began.
struct Vep2Iter {
    VepArgs a;
    Args2 b;
    jrx_stokes2d_fields g;
    const jrx_vep2d_fields *f;       // the caller's arrays

    void adopt_stresses()
    {
        { double *t_ = a.f.txx; a.f.txx = a.txx_out; a.txx_out = t_; }
        { double *t_ = a.f.tyy; a.f.tyy = a.tyy_out; a.tyy_out = t_; }
        b.f.txx = g.txx = a.f.txx; b.f.tyy = g.tyy = a.f.tyy;
    }
    bool odd() const { return a.f.txx != f->txx; }      // an odd number of iterations so far
    // an odd number of swaps: leave τxx, τyy in the caller's arrays, and the arguments pointing at them
    jrx_status restore(jrx_handle *h, hipStream_t s)
    {
        if (!odd()) return JRX_OK;
        const size_t n = (size_t)a.nx * a.ny;
        JRX_HIP(h, hipMemcpyAsync(f->txx, a.f.txx, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(f->tyy, a.f.tyy, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        adopt_stresses();
        return JRX_OK;
    }
};

}   // namespace

extern "C" {

jrx_status jrx_tensor_invariant2d(jrx_handle *h, double *II, const double *xx, const double *yy, const double *xy, int64_t nx, int64_t ny)
{
    if (!h) return JRX_ERR_ARG;
    if (!II || !xx || !yy || !xy || nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "tensor_invariant!: bad argument");
    hipLaunchKernelGGL(k_tensor_invariant2d, dim3((unsigned)((nx * ny + 255) / 256)), dim3(256), 0, h->stream, II, xx, yy, xy, (int)nx, (int)ny);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vep2d_compute_viscosity(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu)
{
    return vep2_viscosity(h, f, rh, p, nu, false);
}
jrx_status jrx_vep2d_compute_viscosity_tauII(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu)
{
    return vep2_viscosity(h, f, rh, p, nu, true);
}

jrx_status jrx_vep2d_update_stresses(jrx_handle *h, const jrx_vep2d_fields *f, const double *theta, double *lambda, double *lambda_v,
                                     const jrx_rheology *rh, const jrx_vep2d_params *p)
{
    JRX_TRY(check_vep(h, f, rh, p));
    if (!theta || !lambda || !lambda_v) return jrx_fail(h, JRX_ERR_ARG, "θ / λ / λv is NULL");
    VepArgs a = make_vep(f, rh, p);
    a.theta = theta; a.lam = lambda; a.lamv = lambda_v;
    const unsigned gv = (unsigned)(((p->nx + 1) * (p->ny + 1) + 255) / 256), gc = (unsigned)((p->nx * p->ny + 255) / 256);
    hipLaunchKernelGGL(k_vep_vertex, dim3(gv), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(k_vep_centre, dim3(gc), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_vep2d_compute_P(jrx_handle *h, const jrx_vep2d_fields *f, double *theta, const jrx_rheology *rh, const jrx_vep2d_params *p)
{
    JRX_TRY(check_vep(h, f, rh, p));
    JRX_TRY(check_vep_thermal(h, f));
    if (!theta) return jrx_fail(h, JRX_ERR_ARG, "θ is NULL");
    const size_t n = (size_t)p->nx * p->ny, nv = (size_t)(p->nx + 1) * (p->ny + 1);
    JRX_TRY(jrx_ensure_etatau(h, 4 * n));
    double *etatau = h->etatau, *Kc = etatau + n, *Gc = Kc + n, *src = f->dT ? Gc + n : nullptr;
    VepArgs a = make_vep(f, rh, p);
    a.theta = theta; a.etatau = etatau; a.Kc = Kc; a.Gc = Gc;
    const unsigned gv = (unsigned)((nv + 255) / 256), gc = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_phase_avg, dim3(gc), dim3(256), 0, h->stream, Kc, Gc, a, false, (double *)nullptr, (double *)nullptr, src);
    JRX_LAUNCH_CHECK(h);
    a.src = src;
    launch_vep_pre(h->stream, gv, a, theta, true, false, h->fused2d_batch && !p->inv_spacing[0]);      // the form the driver takes for constant densities
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_shear2center2d(jrx_handle *h, double *xy_c, const double *xy, int64_t nx, int64_t ny)
{
    if (!h) return JRX_ERR_ARG;
    if (!xy_c || !xy || nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "shear2center!: bad argument");
    hipLaunchKernelGGL(k_epilogue_op2d, dim3((unsigned)((nx * ny + 255) / 256)), dim3(256), 0, h->stream, 0, xy_c, (const double *)nullptr,
                       (const double *)nullptr, xy, 0.0, 0.0, (int)nx, (int)ny);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_accumulate_tensor2d(jrx_handle *h, double *II, const double *xx, const double *yy, const double *xy, double dt, int64_t nx, int64_t ny)
{
    if (!h) return JRX_ERR_ARG;
    if (!II || !xx || !yy || !xy || nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "accumulate_tensor!: bad argument");
    hipLaunchKernelGGL(k_epilogue_op2d, dim3((unsigned)((nx * ny + 255) / 256)), dim3(256), 0, h->stream, 1, II, xx, yy, xy, dt, 0.0, (int)nx, (int)ny);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_compute_vorticity2d(jrx_handle *h, double *wxy, const double *Vx, const double *Vy, int64_t nx, int64_t ny, double _dx, double _dy)
{
    if (!h) return JRX_ERR_ARG;
    if (!wxy || !Vx || !Vy || nx < 1 || ny < 1) return jrx_fail(h, JRX_ERR_ARG, "compute_vorticity!: bad argument");
    hipLaunchKernelGGL(k_epilogue_op2d, dim3((unsigned)(((nx + 1) * (ny + 1) + 255) / 256)), dim3(256), 0, h->stream, 2, wxy, Vx, Vy, (const double *)nullptr,
                       _dx, _dy, (int)nx, (int)ny);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

// accumulate_vol!(EVol_pl, ε_vol_pl, dt): EVol_pl += dt * ε_vol_pl (StressKernels.jl:410-431), any dimension
jrx_status jrx_accumulate_vol(jrx_handle *h, double *EVol, const double *evol, double dt, int64_t n)
{
    if (!h) return JRX_ERR_ARG;
    if (!EVol || !evol || n < 1) return jrx_fail(h, JRX_ERR_ARG, "accumulate_vol!: bad argument");
    hipLaunchKernelGGL(k_axpy_dt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, EVol, evol, dt, (i64)n);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_compute_tau_nonlinear2d(jrx_handle *h, const jrx_vep2d_fields *f, double *theta, double *lambda, const jrx_rheology *rh,
                                       const jrx_vep2d_params *p, int32_t multiphase)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !rh || !p) return jrx_fail(h, JRX_ERR_ARG, "null VEP argument");
    if (p->nx < 1 || p->ny < 1) return jrx_fail(h, JRX_ERR_ARG, "compute_τ_nonlinear!: empty grid");
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
    if (!theta || !lambda) return jrx_fail(h, JRX_ERR_ARG, "θ / λ is NULL");
    const void *req[] = {f->P, f->exx, f->eyy, f->exy, f->eplxx, f->eplyy, f->eplxy, f->txx, f->tyy, f->txy_c, f->tII, f->toxx, f->toyy,
                         f->toxy, f->eta, f->eta_vep, multiphase ? (const void *)f->phase_c : (const void *)f->P};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "compute_τ_nonlinear!: a required field pointer is NULL");
    VepArgs a = make_vep(f, rh, p);
    a.lam = lambda;
    const unsigned gc = (unsigned)((p->nx * p->ny + 255) / 256);
    if (multiphase) hipLaunchKernelGGL(k_tau_nonlinear2d<true>, dim3(gc), dim3(256), 0, h->stream, a, theta);
    else hipLaunchKernelGGL(k_tau_nonlinear2d<false>, dim3(gc), dim3(256), 0, h->stream, a, theta);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_center2vertex2d(jrx_handle *h, double *vertex, const double *center, int64_t nx, int64_t ny)
{
    if (!h) return JRX_ERR_ARG;
    if (!vertex || !center || nx < 2 || ny < 2) return jrx_fail(h, JRX_ERR_ARG, "center2vertex!: bad argument");
    const i64 nv = (nx + 1) * (ny + 1);
    hipLaunchKernelGGL(k_center2vertex2d, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, h->stream, vertex, center, (int)nx, (int)ny, 3);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_stokes2d_vep_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p,
                                  jrx_solve_result *res)
{
    JRX_TRY(check_vep(h, f, rh, p));
    JRX_TRY(check_vep_thermal(h, f));
    if (!res) return jrx_fail(h, JRX_ERR_ARG, "null result");
    if (p->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    const bool comm = jrx_comm_active(h);
    const int nx = (int)p->nx, ny = (int)p->ny;
    const int64_t nn[3] = {nx, ny, 1};
    const size_t n = (size_t)nx * ny, nv = (size_t)(nx + 1) * (ny + 1);
    hipStream_t s = h->stream;
    // library scratch: ητ, θ, λ, K, G (centre), λv (vertex) and the second set of τxx, τyy, carved out of one allocation; with args.ΔT the thermal source of compute_P! behind them
    JRX_TRY(jrx_ensure_etatau(h, (f->dT ? 9 : 8) * n + 2 * nv));
    double *etatau = h->etatau, *theta = etatau + n, *lam = theta + n, *Kc = lam + n, *Gc = Kc + n, *lamv = Gc + n;
    Vep2Iter st;
    st.f = f;
    VepArgs &a = st.a;
    Args2 &b = st.b;
    jrx_stokes2d_fields &g = st.g;
    a = make_vep(f, rh, p);
    a.theta = theta; a.etatau = etatau; a.Kc = Kc; a.Gc = Gc; a.lam = lam; a.lamv = lamv;
    a.txx_out = lamv + nv; a.tyy_out = a.txx_out + n;
    double *eta_lin_c = a.tyy_out + n, *eta_lin_v = eta_lin_c + n;
    double *const src = f->dT ? eta_lin_v + nv : nullptr;
    g = view2d(f);
    jrx_stokes2d_params q;
    memset(&q, 0, sizeof(q));
    q.nx = nx; q.ny = ny; q.nxg = p->nxg; q.nyg = p->nyg; q._dx = p->_dx; q._dy = p->_dy; q.dt = p->dt; q.r = p->r;
    q.theta_dtau = p->theta_dtau; q.eta_dtau = p->eta_dtau; q.free_slip = p->free_slip; q.no_slip = p->no_slip; q.periodic = p->periodic;
    for (int d = 0; d < 6; d++) q.inv_spacing[d] = p->inv_spacing[d];
    b = make_args2(&g, etatau, &q);
    const unsigned gv = (unsigned)((nv + 255) / 256), gc = (unsigned)((n + 255) / 256);

    JRX_HIP(h, hipMemcpyAsync(f->P0, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // @copy stokes.P0 stokes.P
    JRX_HIP(h, hipMemcpyAsync(theta, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // θ = deepcopy(stokes.P)
    JRX_HIP(h, hipMemsetAsync(lam, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(lamv, 0, nv * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxx, 0, n * sizeof(double), s));                                 // @tensor_center(ε_pl) .= 0
    JRX_HIP(h, hipMemsetAsync(f->eplyy, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxy_c, 0, n * sizeof(double), s));
    // linear laws: η of a cell / vertex depends on its phase ratios only -- averaged once per solve, compute_viscosity! then reads one array instead of the ratios
    const bool lin = !a.vfields;
    hipLaunchKernelGGL(k_phase_avg, dim3(lin && f->eta_v ? gv : gc), dim3(256), 0, s, Kc, Gc, a, rh->has_density != 0, lin ? eta_lin_c : (double *)nullptr,
                       lin && f->eta_v ? eta_lin_v : (double *)nullptr, src);
    JRX_LAUNCH_CHECK(h);
    a.src = src;
    if (lin) { a.eta_lin_c = eta_lin_c; a.eta_lin_v = f->eta_v ? eta_lin_v : nullptr; }
    const bool upd_rho = rh->has_density && !mat_density_is_constant(rh);       // update_ρg!: a no-op for constant densities
    const bool ubc = p->displacement_bcs != 0;
    if (ubc) {    // displacement2velocity!(stokes, dt, flow_bcs) (Stokes2D.jl:647): V = U * inv(dt)
        hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Vx, (const double *)f->Ux, (i64)(nx + 1) * (ny + 2), f->Vy,
                           (const double *)f->Uy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, 1.0 / p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    b.fs_dt = p->free_surface ? p->dt : 0.0;      // dt * free_surface with a Bool: Inf * false == 0.0 in Julia (solve! with dt = Inf)
    // option "fused2d_batch" (default): the forms of the pre and viscosity + velocity kernels that request every operand up front -- uniform grids, constant densities, viscosity laws
    // without fields (phase average precomputed), no free surface; everything else keeps the general kernels
    const bool batch_pre = h->fused2d_batch && !p->inv_spacing[0] && !upd_rho;
    const bool batch_vv = h->fused2d_batch && !p->inv_spacing[0] && b.fs_dt == 0.0 && !a.vfields && a.eta_lin_c != nullptr && (a.f.eta_v == nullptr || a.eta_lin_v != nullptr);

    PtLog log(res);
    int64_t iter = 0;
    auto done = [&]() { return log.rel() < p->eps_rel || log.err() < p->eps_abs; };
    auto is_check = [&](int64_t i1) { return (i1 % p->nout == 0) && i1 > 1; };
    // can the loop stop after iteration i1: a check follows it, it is the last allowed one, or the loop has already converged
    auto can_stop = [&](int64_t i1) { return is_check(i1) || i1 > p->iterMax || (p->iterMin < i1 && done()); };
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    // One iteration, enqueued on s, when `iter` are done (the steps marked `comm` only on ranks with neighbours).  diag: a check follows, or the loop can end here -- only
    // then are the output-only arrays stored, is U = V dt observable and does flow_bcs! run as launches of its own
    auto enqueue_iteration = [&](Vep2Iter &it, int64_t iter, bool diag) -> jrx_status {
        VepArgs &A = it.a;
        A.obs = diag || h->vep_store_all;
        if (!diag && h->vep_store_all) h->stat_vep_store_all++;
        if (comm) {
            hipLaunchKernelGGL(k_maxloc, dim3(gc, 1), dim3(256), 0, s, etatau, (const double *)f->eta, nx, ny, 1);
            JRX_LAUNCH_CHECK(h);
            // update_halo!(ητ) (Stokes2D.jl:655)
            double *arrs[1] = {etatau};
            const int64_t ext[1][3] = {{nx, ny, 1}};
            JRX_TRY(jrx_halo_exchange(h, s, 1, arrs, ext, nn));
            launch_vep_pre(s, gv, A, theta, false, upd_rho, false);
        } else launch_vep_pre(s, gv, A, theta, true, upd_rho, batch_pre);
        JRX_LAUNCH_CHECK(h);
        if (A.si) {
            hipLaunchKernelGGL(k_vep_strain_inc, dim3(gv), dim3(256), 0, s, A);
            JRX_LAUNCH_CHECK(h);
        }
        launch_vep_stress2d(h, s, gv, A);      // the new τxx, τyy go to the other set, then swap
        JRX_LAUNCH_CHECK(h);
        it.adopt_stresses();
        if (comm) {   // update_halo!(stokes.τ.xy) (Stokes2D.jl:757)
            double *arrs[1] = {f->txy};
            const int64_t ext[1][3] = {{nx + 1, ny + 1, 1}};
            JRX_TRY(jrx_halo_exchange(h, s, 1, arrs, ext, nn));
        }
        // flow_bcs! applied in full by iteration 1: refresh ghosts in-kernel (never with DisplacementBoundaryConditions: flow_bcs! then acts on U)
        // (nor with strain_increment: U = V dt must copy the ghosts of V as the previous flow_bcs! left them)
        const bool used_bcf = iter >= 1 && p->periodic == 0 && !comm && !ubc && !A.si && !diag;
        // compute_viscosity! + compute_V! (free-surface form with dt*free_surface = 0) in one launch
        if (batch_vv && used_bcf) hipLaunchKernelGGL(k_vep_visc_velocity_b<true>, dim3(gv), dim3(256), 0, s, A, it.b);
        else if (batch_vv) hipLaunchKernelGGL(k_vep_visc_velocity_b<false>, dim3(gv), dim3(256), 0, s, A, it.b);
        else if (used_bcf) hipLaunchKernelGGL(k_vep_visc_velocity<true>, dim3(gv), dim3(256), 0, s, A, it.b);
        else hipLaunchKernelGGL(k_vep_visc_velocity<false>, dim3(gv), dim3(256), 0, s, A, it.b);
        JRX_LAUNCH_CHECK(h);
        if (diag || A.si) {   // U = V*dt is only observable after an iteration the loop can stop at -- or every iteration when the strains are taken from U
            hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Ux, (const double *)f->Vx, (i64)(nx + 1) * (ny + 2), f->Uy,
                               (const double *)f->Vy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, p->dt);
            JRX_LAUNCH_CHECK(h);
        }
        if (ubc) {    // flow_bcs!(stokes, ::DisplacementBoundaryConditions) acts on U = V dt, which the next iteration overwrites: only the last one is observable
            if (diag || A.si) JRX_TRY(jrx2d_bcs(h, s, f->Ux, f->Uy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        } else if (!used_bcf) JRX_TRY(jrx2d_bcs(h, s, f->Vx, f->Vy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        if (comm) {   // update_halo!(@velocity(stokes)...) (Stokes2D.jl:784)
            double *arrs[2] = {f->Vx, f->Vy};
            const int64_t ext[2][3] = {{nx + 1, ny + 2, 1}, {nx + 2, ny + 1, 1}};
            JRX_TRY(jrx_halo_exchange(h, s, 2, arrs, ext, nn));
        }
        return JRX_OK;
    };
    // Runs of unobserved iterations replay as a captured graph of GIT iterations (three launches each: at the sizes where the loop is launch-bound -- 17 - 18 us
    // per iteration up to 256^2 -- the gap between dependent launches is shorter inside a graph).  An even count, so that the (τxx, τyy) sets end where they
    // started; one graph per parity.  Only in the plain steady state: one rank, no periodic face, velocity boundary conditions, strain-rate form.  Option "loop_graphs" = 0: plain launches.
    constexpr int GIT = 32;
    GraphExecs gexec;        // released on every exit path
    bool graphs = h->loop_graphs && !comm && !ubc && !a.si && p->periodic == 0 && (i64)(nx + 1) * (ny + 1) <= 200000;
    while (iter <= p->iterMax) {
        if (p->iterMin < iter && done()) break;          // Stokes2D.jl:650-651
        if (graphs && iter >= 1 && !done()) {
            // observed iterations (checks: multiples of nout; the last one: iterMax + 1) end a run; err does not change inside one
            int64_t run = pt_replay::unobserved_run(iter, p->nout, p->iterMax + 1);
            if (run >= GIT) {
                const int par = st.odd() ? 1 : 0;
                if (!gexec[par]) {
                    JRX_TRY(jrx_capture_graph(s, &gexec[par], [&]() -> jrx_status {
                        Vep2Iter T = st;
                        for (int r_ = 0; r_ < GIT; r_++) JRX_TRY(enqueue_iteration(T, iter + r_, false));
                        return JRX_OK;
                    }));
                    if (!gexec[par]) graphs = false;
                }
                if (gexec[par]) {
                    while (run >= GIT) {
                        JRX_HIP(h, hipGraphLaunch(gexec[par], s));
                        iter += GIT; run -= GIT;
                        h->stat_graph_replays++;
                    }
                    continue;
                }
            }
        }
        JRX_TRY(enqueue_iteration(st, iter, can_stop(iter + 1)));
        iter += 1;
        if (is_check(iter)) {
            hipLaunchKernelGGL(k_velocity2d<true>, dim3(gc), dim3(256), 0, s, b);  // compute_Res!
            JRX_LAUNCH_CHECK(h);
            JRX_TRY(jrx2d_sumsq(h, s, &g, &q));
            double ss[4];
            JRX_TRY(jrx_read_sums(h, s, ss, true));                                      // norm_mpi (Stokes2D.jl:803-808)
            const double nRx = sqrt(ss[0]) / sqrt((double)((p->nxg - 2) * (p->nyg - 1)));
            const double nRy = sqrt(ss[1]) / sqrt((double)((p->nxg - 1) * (p->nyg - 2)));
            const double nDV = sqrt(ss[3]) / sqrt((double)(p->nxg * p->nyg));      // jrx2d_sumsq leaves RP in slot 3
            const double err = log.record(iter, nRx, nRy, nDV);
            if (p->verbose && jrx_comm_rank(h) == 0) log.print2d(iter, nRx, nRy, nDV);      // igg.me == 0 (Stokes2D.jl:814)
            if (std::isnan(err)) {      // error("NaN(s)"): leave the caller's arrays consistent and the stream drained
                gexec.reset();
                (void)st.restore(h, s);
                return log.fail_nan(h, iter, jrx_drain_ms(s, h->ev[6], h->ev[7]));
            }
        }
    }
    gexec.reset();
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    JRX_TRY(st.restore(h, s));
    a.txx_out = a.tyy_out = nullptr;
    hipLaunchKernelGGL(k_vep_epilogue, dim3(gv), dim3(256), 0, s, a);
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

// solve!(stokes, pt_stokes, grid, flow_bcs, ρg, rheology::MaterialParams, args, dt, igg; kwargs) -- src/stokes/Stokes2D.jl:345-557: the
// single-phase visco-elasto-plastic driver, the caller of compute_τ_nonlinear! and center2vertex! (test/test_WENO5.jl:226-291).
// rheology = phase 0 of the table.  compute_P! takes η (not ητ) and updates stokes.P in place (:418-420); θ = P + K dt λ sinψ only
// replaces P after the loop (:523).  The first compute_maxloc! of an iteration (:413) is dead (ητ is recomputed at :437 before its
// only reader, compute_V!) and is not launched.
jrx_status jrx_stokes2d_nonlinear_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p,
                                        jrx_solve_result *res)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !rh || !p || !res) return jrx_fail(h, JRX_ERR_ARG, "null argument");
    JRX_TRY(jrx_check_device(h));
    if (p->nx < 3 || p->ny < 3) return jrx_fail(h, JRX_ERR_ARG, "2D Stokes needs at least 3 cells per dimension");
    if (p->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
    const void *req[] = {f->P, f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Ux, f->Uy, f->exx, f->eyy, f->exy, f->eplxx, f->eplyy, f->eplxy, f->eplxy_c,
                         f->txx, f->tyy, f->txy, f->txy_c, f->tII, f->toxx, f->toyy, f->toxy, f->toxy_c, f->eta, f->eta_vep, f->EII_pl, f->evol_pl,
                         f->EVol_pl, f->fx, f->fy, f->RP, f->Rx, f->Ry};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "a required field pointer is NULL");
    const bool comm = jrx_comm_active(h);
    const int nx = (int)p->nx, ny = (int)p->ny;
    const int64_t nn[3] = {nx, ny, 1};
    const size_t n = (size_t)nx * ny, nv = (size_t)(nx + 1) * (ny + 1);
    hipStream_t s = h->stream;
    JRX_TRY(jrx_ensure_etatau(h, 5 * n));
    double *etatau = h->etatau, *theta = etatau + n, *lam = theta + n, *Kc = lam + n, *Gc = Kc + n;
    VepArgs a = make_vep(f, rh, p);
    a.theta = f->P; a.etatau = f->eta; a.Kc = Kc; a.Gc = Gc; a.lam = lam;          // the view compute_P! works on: P in place, η instead of ητ
    jrx_stokes2d_fields g = view2d(f);
    jrx_stokes2d_params q;
    memset(&q, 0, sizeof(q));
    q.nx = nx; q.ny = ny; q.nxg = p->nxg; q.nyg = p->nyg; q._dx = p->_dx; q._dy = p->_dy; q.dt = p->dt; q.r = p->r;
    q.theta_dtau = p->theta_dtau; q.eta_dtau = p->eta_dtau; q.free_slip = p->free_slip; q.no_slip = p->no_slip; q.periodic = p->periodic;
    for (int d = 0; d < 6; d++) q.inv_spacing[d] = p->inv_spacing[d];
    Args2 b = make_args2(&g, etatau, &q);
    b.fs_dt = p->free_surface ? p->dt : 0.0;      // dt * free_surface with a Bool: Inf * false == 0.0 in Julia (solve! with dt = Inf)
    const unsigned gv = (unsigned)((nv + 255) / 256), gc = (unsigned)((n + 255) / 256);
    const bool tg = p->T_ghosted != 0, ubc = p->displacement_bcs != 0;
    const bool upd_rho = rh->has_density && rh->rho_kind[0] != 0;

    JRX_HIP(h, hipMemsetAsync(theta, 0, n * sizeof(double), s));                                    // θ = @zeros(ni...) :398
    JRX_HIP(h, hipMemsetAsync(lam, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxx, 0, n * sizeof(double), s));                                 // @tensor_center(ε_pl) .= 0 :391-393
    JRX_HIP(h, hipMemsetAsync(f->eplyy, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxy_c, 0, n * sizeof(double), s));
    hipLaunchKernelGGL(k_fill2, dim3(gc), dim3(256), 0, s, Kc, rh->Kb[0], Gc, rh->G[0], (i64)n);      // Kb = get_Kb(rheology); G = get_G(rheology)
    // compute_ρg!(ρg[end], rheology, args); compute_viscosity!(stokes, args, rheology, cutoff) :406-407
    {
        VepArgs a0 = a;
        a0.vtau = false;                    // compute_viscosity! is the εII form; the in-loop compute_viscosity_τII! the τII one
        hipLaunchKernelGGL(k_single_material, dim3(gc), dim3(256), 0, s, a0, 1.0, rh->has_density != 0, true, tg);
    }
    JRX_LAUNCH_CHECK(h);
    if (ubc) {    // displacement2velocity!(stokes, dt, flow_bcs) :410
        hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Vx, (const double *)f->Ux, (i64)(nx + 1) * (ny + 2), f->Vy,
                           (const double *)f->Uy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, 1.0 / p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    PtLog log(res);
    int64_t iter = 0;
    res->iter = 0; res->nchecks = 0;
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    auto keep_going = [&](int64_t it) { return it < 2 || ((log.rel() > p->eps_rel && log.err() > p->eps_abs) && it <= p->iterMax); };
    // Runs of unobserved iterations (ten short launches each as the reference orders them, every argument constant: the loop is launch-bound at any 2D size,
    // 38 us per iteration) replay as a captured graph of GIT iterations of six launches (center2vertex! in one pass, flow_bcs! folded into compute_V!); one rank,
    // velocity boundary conditions.  Option "loop_graphs" = 0: plain launches.
    constexpr int GIT = 16;
    GraphExecs gexecs;       // released on every exit path
    hipGraphExec_t &gexec = gexecs[0];
    bool graphs = h->loop_graphs && !comm && !ubc;
    // One iteration, enqueued on s (the exchanges only on ranks with neighbours).  diag: a check follows, or the loop ends here -- U is only observable then.  folded: the form
    // a replay takes -- flow_bcs! has been applied in full by then (iter >= 2), so without a periodic face the velocity kernel refreshes the ghosts next to what it updates
    // and no flow_bcs! launch follows
    auto enqueue_iteration = [&](bool diag, bool folded) -> jrx_status {
        hipLaunchKernelGGL(k_vep_pre<false>, dim3(gv), dim3(256), 0, s, a, f->P);                    // compute_∇V!, compute_P!, compute_strain_rate!
        hipLaunchKernelGGL(k_single_material, dim3(gc), dim3(256), 0, s, a, p->viscosity_relaxation, upd_rho, true, tg);   // update_ρg!, compute_viscosity_τII!
        hipLaunchKernelGGL(k_maxloc, dim3(gc, 1), dim3(256), 0, s, etatau, (const double *)f->eta, nx, ny, 1);            // compute_maxloc!(ητ, η) :437
        JRX_LAUNCH_CHECK(h);
        if (comm) {
            double *arrs[1] = {etatau};
            const int64_t ext[1][3] = {{nx, ny, 1}};
            JRX_TRY(jrx_halo_exchange(h, s, 1, arrs, ext, nn));
        }
        hipLaunchKernelGGL(k_tau_nonlinear2d<false>, dim3(gc), dim3(256), 0, s, a, theta);           // compute_τ_nonlinear! :440-458
        hipLaunchKernelGGL(k_center2vertex2d, dim3(gv), dim3(256), 0, s, f->txy, (const double *)f->txy_c, nx, ny, 3);   // center2vertex! :459, its three passes in one
        JRX_LAUNCH_CHECK(h);
        if (comm) {   // update_halo!(stokes.τ.xy) :460
            double *arrs[1] = {f->txy};
            const int64_t ext[1][3] = {{nx + 1, ny + 1, 1}};
            JRX_TRY(jrx_halo_exchange(h, s, 1, arrs, ext, nn));
        }
        const bool bcf = folded && p->periodic == 0;
        if (bcf) hipLaunchKernelGGL((k_velocity2d<false, true>), dim3(gc), dim3(256), 0, s, b);
        else hipLaunchKernelGGL(k_velocity2d<false>, dim3(gc), dim3(256), 0, s, b);                  // compute_V! (free-surface form) :463-474
        JRX_LAUNCH_CHECK(h);
        if (diag) {
            hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Ux, (const double *)f->Vx, (i64)(nx + 1) * (ny + 2), f->Uy,
                               (const double *)f->Vy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, p->dt);
            JRX_LAUNCH_CHECK(h);
        }
        if (ubc) {
            if (diag) JRX_TRY(jrx2d_bcs(h, s, f->Ux, f->Uy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        } else if (!bcf) JRX_TRY(jrx2d_bcs(h, s, f->Vx, f->Vy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        if (comm) {
            double *arrs[2] = {f->Vx, f->Vy};
            const int64_t ext[2][3] = {{nx + 1, ny + 2, 1}, {nx + 2, ny + 1, 1}};
            JRX_TRY(jrx_halo_exchange(h, s, 2, arrs, ext, nn));
        }
        return JRX_OK;
    };
    while (keep_going(iter)) {
        if (graphs && iter >= 2) {
            int64_t run = pt_replay::unobserved_run(iter, p->nout, p->iterMax + 1);      // observed: the multiples of nout and iteration iterMax + 1
            if (run >= GIT) {
                if (!gexec) {
                    JRX_TRY(jrx_capture_graph(s, &gexec, [&]() -> jrx_status {
                        for (int r_ = 0; r_ < GIT; r_++) JRX_TRY(enqueue_iteration(false, true));
                        return JRX_OK;
                    }));
                    if (!gexec) graphs = false;
                }
                if (gexec) {
                    while (run >= GIT) {
                        JRX_HIP(h, hipGraphLaunch(gexec, s));
                        iter += GIT; run -= GIT;
                        h->stat_graph_replays++;
                    }
                    continue;
                }
            }
        }
        const int64_t it1 = iter + 1;
        const bool check = (it1 % p->nout == 0) && it1 > 1;
        JRX_TRY(enqueue_iteration(check || !keep_going(it1), false));      // U is only observable after an iteration a check follows or the loop ends at
        iter = it1;
        if (check) {
            hipLaunchKernelGGL(k_velocity2d<true>, dim3(gc), dim3(256), 0, s, b);                    // compute_Res! :479-490
            JRX_LAUNCH_CHECK(h);
            JRX_TRY(jrx2d_sumsq(h, s, &g, &q));
            double ss[4];
            JRX_TRY(jrx_read_sums(h, s, ss, true));
            const double nRx = sqrt(ss[0]) / sqrt((double)((p->nxg - 2) * (p->nyg - 1)));
            const double nRy = sqrt(ss[1]) / sqrt((double)((p->nxg - 1) * (p->nyg - 2)));
            const double nDV = sqrt(ss[3]) / sqrt((double)(p->nxg * p->nyg));      // jrx2d_sumsq leaves RP in slot 3
            const double err = log.record(iter, nRx, nRy, nDV);
            if (jrx_comm_rank(h) == 0 && ((p->verbose && log.rel() > p->eps_rel && err > p->eps_abs) || iter == p->iterMax)) log.print2d(iter, nRx, nRy, nDV);
            if (std::isnan(err)) return log.fail_nan(h, iter, jrx_drain_ms(s, h->ev[6], h->ev[7]));
        }
    }
    gexecs.reset();
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    JRX_HIP(h, hipMemcpyAsync(f->P, theta, n * sizeof(double), hipMemcpyDeviceToDevice, s));        // stokes.P .= θ :523
    a.txx_out = a.tyy_out = nullptr;
    hipLaunchKernelGGL(k_vep_epilogue, dim3(gv), dim3(256), 0, s, a);
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
