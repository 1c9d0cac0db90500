// jrx_material.hpp -- per-phase material laws of the rheology table (jrx_rheology): density, strain softening, creep viscosity, and the
// plasticity helpers of rheology/StressUpdate.jl that the 2D and 3D visco-elasto-plastic drivers share (one copy: stokes2d_vep.hip, stokes3d_vep.hip).
// The reference delegates these to GeoParams.jl (compute_density, softening_C / softening_ϕ, compute_viscosity_τII; call sites
// rheology/BuoyancyForces.jl:37-60, rheology/StressUpdate.jl:305-381, rheology/Viscosity.jl:142-167); the forms are stated in include/jrx.h.
#pragma once
#include "jrx_internal.hpp"

__device__ __forceinline__ double mat_density(const jrx_rheology &rh, int q, double T, double P)
{
    switch (rh.rho_kind[q]) {
    case 1: return rh.rho0[q] * (1.0 - rh.alpha[q] * (T - rh.T0[q]) + rh.beta[q] * (P - rh.P0[q]));
    case 2: return rh.rho0[q] * (1.0 - rh.alpha[q] * (T - rh.T0[q]));
    case 3: return rh.rho0[q] * exp(rh.beta[q] * (P - rh.P0[q]));
    default: return rh.rho0[q];
    }
}
// fn_ratio(compute_density, rheology, ratio, args) -- src/phases/phases.jl:17-30
__device__ __forceinline__ double mat_density_ratio(const jrx_rheology &rh, const double *r, double T, double P)
{
    double x = 0.0;
    for (int q = 0; q < rh.nphase; q++) {
        const double rq = r[q];
        if (rq == 1.0) return mat_density(rh, q, T, P) * rq;
        x += (rq == 0.0) ? 0.0 : mat_density(rh, q, T, P) * rq;
    }
    return x;
}
// get_thermal_expansion of a phase: the α of its density law (PT_Density, T_Density), 0 for the laws without one [GeoParams form, assumed; include/jrx.h]
__device__ __forceinline__ double mat_thermal_expansion(const jrx_rheology &rh, int q)
{
    return (rh.rho_kind[q] == 1 || rh.rho_kind[q] == 2) ? rh.alpha[q] : 0.0;
}
// fn_ratio(get_thermal_expansion, rheology, ratio) with the rules of mat_density_ratio (zero ratios skipped, a ratio of one returns that phase's value alone).  The early return is this
// project's choice: PressureKernels.jl:147 calls the three-argument fn_ratio (src/phases/phases.jl:6-15), which only skips zero ratios.  The two differ only when a ratio of exactly 1
// follows a non-zero ratio, i.e. never for ratios that sum to one.
__device__ __forceinline__ double mat_thermal_expansion_ratio(const jrx_rheology &rh, const double *r)
{
    double x = 0.0;
    for (int q = 0; q < rh.nphase; q++) {
        const double rq = r[q];
        if (rq == 1.0) return mat_thermal_expansion(rh, q) * rq;
        x += (rq == 0.0) ? 0.0 : mat_thermal_expansion(rh, q) * rq;
    }
    return x;
}
static inline bool mat_density_is_constant(const jrx_rheology *rh)
{
    for (int q = 0; q < rh->nphase; q++)
        if (rh->rho_kind[q] != 0) return false;
    return true;
}
static inline bool mat_has_softening(const jrx_rheology *rh)
{
    for (int q = 0; q < rh->nphase; q++)
        if (rh->softC_kind[q] != 0 || rh->softphi_kind[q] != 0) return true;
    return false;
}

__device__ __forceinline__ double mat_soften(int kind, double a, double b, double c, double d, double EII, double v0)
{
    if (kind == 1) {
        if (EII >= d) return a;
        if (EII <= c) return b;
        return b + (a - b) / (d - c) * (EII - c);
    }
    if (kind == 2) return a - 0.5 * b * erfc(-(EII - c) / d);
    return v0;
}
__device__ __forceinline__ double mat_cohesion(const jrx_rheology &rh, int q, double EII)
{
    return mat_soften(rh.softC_kind[q], rh.softC_a[q], rh.softC_b[q], rh.softC_c[q], rh.softC_d[q], EII, rh.C[q]);
}
__device__ __forceinline__ void mat_friction(const jrx_rheology &rh, int q, double EII, double &sinphi, double &cosphi)
{
    if (rh.softphi_kind[q] == 0) { sinphi = rh.sinphi[q]; cosphi = rh.cosphi[q]; return; }
    const double phi = mat_soften(rh.softphi_kind[q], rh.softphi_a[q], rh.softphi_b[q], rh.softphi_c[q], rh.softphi_d[q], EII, rh.phi_deg[q]);
    const double rad = phi * (3.14159265358979323846 / 180.0);
    sinphi = sin(rad); cosphi = cos(rad);
}
__device__ __forceinline__ double mat_creep_viscosity(const jrx_rheology &rh, int q, double T, double P)
{
    if (rh.visc_kind[q] == 1) {
        const double e = rh.eta[q] * exp((rh.Ea[q] + P * rh.Va[q]) / (rh.Rgas[q] * T) - rh.Ea[q] / (rh.Rgas[q] * rh.Tref[q]));
        return fmin(fmax(e, rh.visc_lo[q]), rh.visc_hi[q]);
    }
    return rh.eta[q];
}
// fn_viscosity(rheology[q].CompositeRheology[1], AII, args): AII is a stress invariant (compute_viscosity_τII, tau = true) or a strain-rate invariant
// (compute_viscosity_εII); only the power-law creep (visc_kind 2) reads it
__device__ __forceinline__ double mat_viscosity(const jrx_rheology &rh, int q, double AII, double T, double P, bool tau)
{
    if (rh.visc_kind[q] != 2) return mat_creep_viscosity(rh, q, T, P);
    const double n = rh.creep_n[q], H = rh.Ea[q] + P * rh.Va[q], RT = rh.Rgas[q] * T;
    if (tau) {
        const double eps = rh.creep_A[q] * pow(AII * rh.creep_FT[q], n) * exp(-H / RT) / rh.creep_FE[q];
        return 0.5 * AII / eps;
    }
    const double t = pow(rh.creep_A[q], -1.0 / n) * pow(AII * rh.creep_FE[q], 1.0 / n) * exp(H / (n * RT)) / rh.creep_FT[q];
    return 0.5 * t / AII;
}
// compute_phase_viscosity (rheology/Viscosity.jl:599-619): a phase above 0.999 alone, else the ratio-weighted harmonic mean
__device__ __forceinline__ double mat_phase_viscosity(const jrx_rheology &rh, const double *r, double AII, double T, double P, bool tau)
{
    for (int q = 0; q < rh.nphase; q++)
        if (r[q] > 0.999) return mat_viscosity(rh, q, AII, T, P, tau);
    double s = 0.0;
    for (int q = 0; q < rh.nphase; q++)
        if (r[q] != 0.0) s += (1.0 / mat_viscosity(rh, q, AII, T, P, tau)) * r[q];
    return 1.0 / s;
}
// the invariant the viscosity kernels form from (xx, yy, xy) (Viscosity.jl:394-404): eps() on the normal components of an all-zero tensor
__device__ __forceinline__ double mat_visc_invariant2(double xx, double yy, double xy)
{
    const double a0 = (xx == 0.0 && yy == 0.0 && xy == 0.0) ? 2.220446049250313e-16 : 0.0;
    const double x = a0 + xx, y = -a0 + yy;
    return sqrt(0.5 * (x * x + y * y) + xy * xy);
}
__host__ __device__ static inline bool mat_viscosity_reads_fields(const jrx_rheology *rh)
{
    for (int q = 0; q < rh->nphase; q++)
        if (rh->visc_kind[q] != 0) return true;
    return false;
}
__host__ __device__ static inline bool mat_viscosity_reads_invariant(const jrx_rheology *rh)
{
    for (int q = 0; q < rh->nphase; q++)
        if (rh->visc_kind[q] == 2) return true;
    return false;
}

// ---- plasticity (rheology/StressUpdate.jl), as update_stresses_center_vertex_ps! 2D and 3D use it

// second invariant of a deviatoric tensor: (xx, yy, xy) in 2D, (xx, yy, zz, yz, xz, xy) in 3D
__device__ __forceinline__ double sinv2(double xx, double yy, double xy) { return sqrt(0.5 * (xx * xx + yy * yy) + xy * xy); }
__device__ __forceinline__ double sinv3(const double t[6])
{
    return sqrt(0.5 * (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + t[3] * t[3] + t[4] * t[4] + t[5] * t[5]);
}
// fn_ratio, src/phases/phases.jl:6-15
// UNROLL: `#pragma unroll` on the phase loop.  The 3D kernels have it, the 2D ones do not, and each side keeps what it was tuned with: with the pragma the 2D kernels
// that take the phase count at run time grow by 12 - 30 % in instructions (k_vep_vertex 5,893 -> 6,900 lines of ISA, k_phase_avg 890 -> 1,170)
template <bool UNROLL = false>
__device__ __forceinline__ double ratio_avg(const double *val, const double *r, int n)
{
    double x = 0.0;
    if (UNROLL) {
#pragma unroll
        for (int q = 0; q < n; q++) x += (r[q] == 0.0) ? 0.0 : val[q] * r[q];
    } else {
        for (int q = 0; q < n; q++) x += (r[q] == 0.0) ? 0.0 : val[q] * r[q];
    }
    return x;
}
// NP > 0: the number of phases as a compile-time constant (the phase loops unroll and the caller hands the ratios in registers, loaded in one batch), else rh.nphase
template <int NP = 0>
__device__ __forceinline__ void plastic_params(const jrx_rheology &rh, const double *r, bool &is_pl, double &eta_reg)
{   // plastic_params_phase, rheology/StressUpdate.jl:152-176
    is_pl = false; eta_reg = 0.0;
    const int np = NP > 0 ? NP : rh.nphase;
#pragma unroll
    for (int q = 0; q < np; q++)
        if (rh.is_pl[q]) { is_pl = true; eta_reg += rh.eta_vp[q] * r[q]; }
}
// SOFT: some phase has a softening law (compiled out otherwise: the erfc / sincos paths cost the 3D edge kernel its second wave per SIMD)
template <bool SOFT, int NP = 0>
__device__ __forceinline__ double yield_F(const jrx_rheology &rh, const double *r, double P, double tII, double EII)
{   // compute_yieldfunction_phase, StressUpdate.jl:399-410 (2D), :435-452 (3D) ; DP: F = τII - cosϕ(EII) C(EII) - sinϕ(EII) P (softening at the EII keyword)
    double F = 0.0;
    const int np = NP > 0 ? NP : rh.nphase;
#pragma unroll
    for (int q = 0; q < np; q++) {
        if (r[q] == 0.0) continue;
        double Fq = tII;
        if (rh.is_pl[q]) {
            if (SOFT) {
                double sp, cp;
                mat_friction(rh, q, EII, sp, cp);
                Fq = tII - cp * mat_cohesion(rh, q, EII) - sp * P;
            } else Fq = tII - rh.cosphi[q] * rh.C[q] - rh.sinphi[q] * P;
        }
        F += r[q] * Fq;
    }
    return F;
}
// NN normal components followed by NC - NN shear components: 2, 3 in 2D and 3, 6 in 3D
template <int NN, int NC, int NP = 0>
__device__ __forceinline__ void plastic_grad(const jrx_rheology &rh, const double *r, const double t[NC], double dQdt[NC], double &dQdP, double &dFdP)
{   // compute_plastic_gradients_phase, StressUpdate.jl:476-495 (2D), :463-550 (3D; shear slots halved once, :466-472) ; ∂Q/∂τ = τ/(2 τII), ∂Q/∂P = -sinψ, ∂F/∂P = -sinϕ
    static_assert((NN == 2 && NC == 3) || (NN == 3 && NC == 6), "2D or 3D tensor");
#pragma unroll
    for (int q = 0; q < NC; q++) dQdt[q] = 0.0;
    dQdP = 0.0; dFdP = 0.0;
    double tII;
    if constexpr (NC == 3) tII = sinv2(t[0], t[1], t[2]);
    else tII = sinv3(t);
    const int np = NP > 0 ? NP : rh.nphase;
    // ∂Q/∂τ of a Drucker-Prager phase does not depend on the phase: one division per component instead of one per component and phase (the same quotient, so the same bits)
    bool any_pl = false;
#pragma unroll
    for (int q = 0; q < np; q++) any_pl |= rh.is_pl[q] != 0;
    double g[NC] = {};
    if (any_pl) {
#pragma unroll
        for (int s = 0; s < NN; s++) g[s] = 0.5 * t[s] / tII;
#pragma unroll
        for (int s = NN; s < NC; s++) g[s] = 0.5 * (t[s] / tII);
    }
#pragma unroll
    for (int q = 0; q < np; q++) {
        if (r[q] == 0.0 || !rh.is_pl[q]) continue;
#pragma unroll
        for (int s = 0; s < NC; s++) dQdt[s] = fma(r[q], g[s], dQdt[s]);
        dQdP = fma(r[q], -rh.sinpsi[q], dQdP);
        dFdP = fma(r[q], -rh.sinphi[q], dFdP);
    }
}
