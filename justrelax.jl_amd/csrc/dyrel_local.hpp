// dyrel_local.hpp -- the local constitutive law of DYREL, shared by dyrel2d.hip (NC = 3 components: xx, yy, xy) and dyrel3d.hip (NC = 6: xx, yy, zz, yz, xz, xy).
//
// Reference (PTsolvers/JustRelax.jl): src/DYREL/stress_kernels.jl:224-315 (compute_local_stress, _compute_local_stress, empty_stress_solution for 3- and 6-tuples)
// and :129-135 (_update_τII_viscosity).  The reference's text is written for a tuple of any length; the component count is the template parameter here.
// The NC = 3 instantiation is the arithmetic dyrel2d.hip carried before this header existed, operation for operation.
#pragma once
#include "jrx_material.hpp"

namespace {

// what compute_local_stress returns: τ (NC), ε_pl (NC), then τII, λ, ΔPψ, η_vep, ε_vol_pl -- 11 values for NC = 3, 17 for NC = 6
template <int NC>
struct DyLocal {
    double v[2 * NC + 5];
    static constexpr int TII = 2 * NC, LAM = 2 * NC + 1, DP = 2 * NC + 2, VEP = 2 * NC + 3, EVOL = 2 * NC + 4;
};

// second_invariant of a 3- or 6-tuple, normal components first
template <int NC>
__device__ __forceinline__ double dy_sinv(const double t[NC])
{
    static_assert(NC == 3 || NC == 6, "2D or 3D tensor");
    if constexpr (NC == 3) return sinv2(t[0], t[1], t[2]);
    else return sinv3(t);
}

// compute_local_stress (stress_kernels.jl:224-247) with _compute_local_stress (:249-307) per phase: ratio .* result, summed in phase order
template <bool SOFT, int NC>
__device__ __forceinline__ DyLocal<NC> dy_local_stress(const jrx_rheology &rh, const double *__restrict__ r, const double e[NC], const double to[NC], const double eta,
                                                       const double P, const double lam, const double rel, const double dt, const double EII)
{
    constexpr int NN = NC == 3 ? 2 : 3, NO = 2 * NC + 5;
    typedef DyLocal<NC> L;
    L acc;
#pragma unroll
    for (int s = 0; s < NO; s++) acc.v[s] = 0.0;
    const double eII_in = dy_sinv<NC>(e);
    for (int q = 0; q < rh.nphase; q++) {
        const double rq = r[q];
        double o[NO];
#pragma unroll
        for (int s = 0; s < NO; s++) o[s] = 0.0;      // empty_stress_solution / the early return
        if (rq != 0.0) {
            const double G = rh.G[q], Kb = rh.Kb[q];
            const bool ispl = rh.is_pl[q] != 0;
            const double eta_reg = ispl ? rh.eta_vp[q] : 0.0;
            const double eta_ve = isinf(G) ? 1.0 / (1.0 / eta + 1.0 / (G * dt)) : (eta * G * dt) / (eta + G * dt);
            const double inv_2Gdt = 1.0 / (2 * G * dt);
            double f[NC];
#pragma unroll
            for (int s = 0; s < NC; s++) f[s] = e[s] + to[s] * inv_2Gdt;
            if (dy_sinv<NC>(f) == 0.0) o[L::VEP] = eta;
            else {
                double t[NC], g[NC];
#pragma unroll
                for (int s = 0; s < NC; s++) { t[s] = 2 * eta_ve * f[s]; g[s] = 0.0; }
                double tII = dy_sinv<NC>(t);
                double F = tII, dQdP = 0.0, dFdP = 0.0;
                if (ispl) {      // Drucker-Prager: F = τII - cosϕ(EII) C(EII) - sinϕ(EII) P; ∂Q/∂τ = τ / (2 τII), shear slots halved once; ∂Q/∂P = -sinψ; ∂F/∂P = -sinϕ
                    double sp = rh.sinphi[q], cp = rh.cosphi[q], C = rh.C[q];
                    if (SOFT) { mat_friction(rh, q, EII, sp, cp); C = mat_cohesion(rh, q, EII); }
                    F = tII - cp * C - sp * P;
#pragma unroll
                    for (int s = 0; s < NN; s++) g[s] = 0.5 * t[s] / tII;
#pragma unroll
                    for (int s = NN; s < NC; s++) g[s] = 0.5 * (t[s] / tII);
                    dQdP = -rh.sinpsi[q]; dFdP = -rh.sinphi[q];
                }
                double l = 0.0, evol = 0.0;
                if (ispl && F >= 0) {
                    const double bulk = isinf(Kb) ? 0.0 : Kb * dt * dFdP * dQdP;
                    const double lnew = F / (eta_ve + eta_reg + bulk);
                    l = rel * lnew + (1 - rel) * lam;
                    evol = -l * dQdP;
                }
                double p[NC], dP = 0.0;
#pragma unroll
                for (int s = 0; s < NC; s++) p[s] = 0.0;
                if (l > 0) {
#pragma unroll
                    for (int s = 0; s < NC; s++) { p[s] = l * g[s]; t[s] = t[s] - 2.0 * eta_ve * p[s]; }
                    tII = dy_sinv<NC>(t);
                    dP = dQdP == 0.0 ? 0.0 : -l * dQdP * Kb * dt;
                }
#pragma unroll
                for (int s = 0; s < NC; s++) { o[s] = t[s]; o[NC + s] = p[s]; }
                o[L::TII] = tII; o[L::LAM] = l; o[L::DP] = dP;
                o[L::VEP] = tII * 0.5 * (1.0 / eII_in);
                o[L::EVOL] = evol;
            }
#pragma unroll
            for (int s = 0; s < NO; s++) o[s] = rq * o[s];
        }
#pragma unroll
        for (int s = 0; s < NO; s++) acc.v[s] = q == 0 ? o[s] : acc.v[s] + o[s];
    }
    return acc;
}

// the invariant _update_τII_viscosity forms (stress_kernels.jl:130-131): allzero(τ...) * eps() on the normal components.  NC = 3: (τxx + ε, τyy - ε, τxy).
// NC = 6 has no reference text: the guard is taken over all six components and spread as compute_viscosity_kernel! 3D spreads it (rheology/Viscosity.jl:481-492):
// (τxx + ε, τyy - ε/2, τzz - ε/2), so the tensor stays deviatoric
template <int NC>
__device__ __forceinline__ double dy_visc_invariant(const double t[NC])
{
    if constexpr (NC == 3) return mat_visc_invariant2(t[0], t[1], t[2]);
    else {
        const bool zero = t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0 && t[3] == 0.0 && t[4] == 0.0 && t[5] == 0.0;
        const double a0 = zero ? 2.220446049250313e-16 : 0.0;
        const double q[6] = {t[0] + a0, t[1] + -a0 * 0.5, t[2] + -a0 * 0.5, t[3], t[4], t[5]};
        return sinv3(q);
    }
}

// _update_τII_viscosity (stress_kernels.jl:129-135): the creep viscosity at the invariant of the fresh stress, continuation_linear with the old value, cutoff
template <int NC>
__device__ __forceinline__ double dy_visc(const jrx_rheology &rh, const double nu, const double cut_lo, const double cut_hi, const double *r, const double t[NC],
                                          const double T, const double P, const double eta_old)
{
    const double tII = dy_visc_invariant<NC>(t);
    const double e = mat_phase_viscosity(rh, r, tII, T, P, true);
    const double x = (1 - nu) * eta_old + nu * e;
    return fmin(fmax(x, cut_lo), cut_hi);
}

}   // namespace
