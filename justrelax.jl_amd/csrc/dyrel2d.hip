// dyrel2d.hip -- 2D DYREL (self-tuned dynamic relaxation inside Powell-Hestenes pressure iterations) for gfx950: kernels, per-kernel entry points, driver.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/DYREL/solver.jl:44-294 (_solve_DYREL!; here its prologue :86-117, the loop is dyrel_common.hpp's),
// pressure_kernels.jl:112 (_compute_RP!, the plain form of _RP_cell :118-121), velocity_kernels.jl:154-240 (compute_∇V_strain_rate_RP!), :326-349
// (compute_PH_residual_V!), :660-727 (damped_update_V, compute_DR_residual_update_V!), stress_kernels.jl:100-307 (compute_stress_viscosity_DRYEL!,
// compute_local_stress, _compute_local_stress), Gershgorin.jl:1-155 (Gershgorin_Stokes2D_SchurComplement!).
// Shared with dyrel3d.hip: the sums, the check-time kernels, DYREL! and the solve loop (dyrel_common.hpp), its error bookkeeping (dyrel_conv.hpp), the local law
// (dyrel_local.hpp).
//
// One inner iteration is three launches, as the reference fuses it: k_dy_strain_rp -> k_dy_stress -> k_dy_update.
// Hazards of the stress kernel (the reference's ordering is stress, halo, viscosity): every array it writes -- τ (xx, yy, xy_c, xx_v, yy_v, xy), ε_pl, ε_vol_pl,
// τII, η_vep, λ, λv, ΔPψ, θc, η, ηv -- is read by the same launch at the thread's own index only (η[I], ηv[I], λ[I], λv[I]); what it reads at neighbours (ε.xx, ε.yy,
// ε.xy, P, EII_pl, and P / T for the viscosity arguments) it never writes.  The viscosity refresh reads the in-register stress of the own node.  So η needs no
// second set here (k_vs_pre does: compute_maxloc! reads the neighbours' η).  The Gershgorin estimate, which does read η and ηv at neighbours, is its own launch.
//
// The per-phase laws (cohesion and friction softening, creep viscosity, the phase average of the viscosity, fn_ratio) are jrx_material.hpp's.  Its phase-weighted
// plasticity helpers (plastic_params, yield_F, plastic_grad) average the PARAMETERS over the phases of a node; DYREL's compute_local_stress evaluates the whole
// return mapping per phase and averages the RESULTS, so those three do not apply: the yield function and the flow direction of one phase are formed here from
// the same per-phase laws.  32-bit element offsets (the extents are checked against 2^31).
// Not built here: 3D (dyrel3d.hip), more than one rank, non-uniform spacing, a RockRatio, the thermal / melt-fraction forms of _RP_cell.
#include "dyrel_common.hpp"
#include "dyrel_local.hpp"
#include "stokes2d_kernels.hpp"

namespace {

struct DyArgs {
    jrx_vep2d_fields f;
    jrx_dyrel2d_fields d;
    jrx_rheology rh;
    double _dx, _dy, dt, rel, nu, cut_lo, cut_hi;
    int nx, ny;
    unsigned fs, ns;
    bool tg;
};

#define C2(A, i_, j_) (A)[(i_) + nx * (j_)]
#define V2(A, i_, j_) (A)[(i_) + (nx + 1) * (j_)]

// compute_∇V_strain_rate_RP! (velocity_kernels.jl:180-240): one thread per vertex index (i, j) of (nx+1, ny+1); ∇V stays in a register
template <bool STRAIN>
__global__ __launch_bounds__(256) void k_dy_strain_rp(double *__restrict__ exx, double *__restrict__ eyy, double *__restrict__ exy, const double *__restrict__ Vx,
                                                      const double *__restrict__ Vy, double *__restrict__ RP, const double *__restrict__ P,
                                                      const double *__restrict__ P0, const double *__restrict__ Q, const double *__restrict__ etab,
                                                      const double _dx, const double _dy, const double dt, const int nx, const int ny)
{
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
#define VX(i_, j_) Vx[(i_) + (nx + 1) * (j_)]
#define VY(i_, j_) Vy[(i_) + (nx + 2) * (j_)]
    const double vx_n = VX(i, j + 1), vy_e = VY(i + 1, j);
    if (STRAIN) {
        const double dVx_dy = (vx_n - VX(i, j)) * _dy, dVy_dx = (vy_e - VY(i, j)) * _dx;
        exy[t] = 0.5 * (dVx_dy + dVy_dx);
    }
    if (i < nx && j < ny) {
        const int c = i + nx * j;
        const double dVx_dx = (VX(i + 1, j + 1) - vx_n) * _dx, dVy_dy = (VY(i + 1, j + 1) - vy_e) * _dy;
        const double div = dVx_dx + dVy_dy;
        if (STRAIN) {
            const double div_third = div * (1.0 / 3.0);
            exx[c] = dVx_dx - div_third;
            eyy[c] = dVy_dy - div_third;
        }
        RP[c] = -div - (P[c] - P0[c]) / etab[c] + (Q[c] / dt);      // _compute_RP!, pressure_kernels.jl:112
    }
#undef VX
#undef VY
}

// the local law (compute_local_stress, _update_τII_viscosity) is dyrel_local.hpp's, with NC = 3 components (xx, yy, xy): 11 values per node
// compute_stress_viscosity_DRYEL! (stress_kernels.jl:137-222): one thread per vertex index; the vertex half, then the centre half of the cell with the same index
template <bool SOFT, bool LIN>
__global__ __launch_bounds__(256) void k_dy_stress(const DyArgs a)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ P = a.f.P, *__restrict__ exx = a.f.exx, *__restrict__ eyy = a.f.eyy, *__restrict__ exy = a.f.exy, *__restrict__ EIIa = a.f.EII_pl;
    const bool vfields = mat_viscosity_reads_fields(&a.rh);
    {   // vertex (i, j): clamped_indices / av_clamped (StressKernels.jl:1304-1315)
        const int i0 = clampi(i - 1, 0, nx - 1), ic = clampi(i, 0, nx - 1), j0 = clampi(j - 1, 0, ny - 1), jc = clampi(j, 0, ny - 1);
#define AVC(A) (0.25 * (C2(A, i0, j0) + C2(A, ic, jc) + C2(A, i0, jc) + C2(A, ic, j0)))
        const double e0 = AVC(exx), e1 = AVC(eyy), Pv = AVC(P), EIIv = AVC(EIIa);
#undef AVC
        const double etav = a.f.eta_v[t];
        const double *rv = a.f.phase_v + np * t;
        const double ev[3] = {e0, e1, exy[t]}, tov[3] = {a.d.toxx_v[t], a.d.toyy_v[t], a.f.toxy[t]};
        const DyLocal<3> o = dy_local_stress<SOFT, 3>(a.rh, rv, ev, tov, etav, Pv, a.d.lambda_v[t], a.rel, a.dt, EIIv);
        a.d.txx_v[t] = o.v[0]; a.d.tyy_v[t] = o.v[1]; a.f.txy[t] = o.v[2];
        a.f.eplxy[t] = o.v[5];
        a.d.lambda_v[t] = o.v[7];
        if (!LIN) {
            double T = 0.0;      // local_viscosity_args_vertex (Viscosity.jl:526-548): T and P averaged over the clamped cells around the vertex
            if (vfields && a.f.T) {
                if (a.tg) { const double *q = a.f.T + i + (nx + 2) * j; T = 0.25 * (q[0] + q[1] + q[nx + 2] + q[nx + 3]); }
                else T = 0.25 * (C2(a.f.T, i0, j0) + C2(a.f.T, ic, j0) + C2(a.f.T, i0, jc) + C2(a.f.T, ic, jc));
            }
            const double Pa = vfields ? 0.25 * (C2(P, i0, j0) + C2(P, ic, j0) + C2(P, i0, jc) + C2(P, ic, jc)) : 0.0;
            a.f.eta_v[t] = dy_visc<3>(a.rh, a.nu, a.cut_lo, a.cut_hi, rv, o.v, T, Pa, etav);
        }
    }
    if (i < nx && j < ny) {      // centre (i, j)
        const int c = i + nx * j;
        const double e2 = (V2(exy, i, j) + V2(exy, i + 1, j) + V2(exy, i, j + 1) + V2(exy, i + 1, j + 1)) / 4;      // sum(_gather(ε.xy)) / 4
        const double eta = a.f.eta[c], Pc = P[c];
        const double *rc = a.f.phase_c + np * c;
        const double ec[3] = {exx[c], eyy[c], e2}, toc[3] = {a.f.toxx[c], a.f.toyy[c], a.f.toxy_c[c]};
        const DyLocal<3> o = dy_local_stress<SOFT, 3>(a.rh, rc, ec, toc, eta, Pc, a.d.lambda[c], a.rel, a.dt, EIIa[c]);
        a.f.txx[c] = o.v[0]; a.f.tyy[c] = o.v[1]; a.f.txy_c[c] = o.v[2];
        a.f.eplxx[c] = o.v[3]; a.f.eplyy[c] = o.v[4];
        a.f.evol_pl[c] = o.v[10];
        a.f.tII[c] = o.v[6];
        a.f.eta_vep[c] = o.v[9];
        a.d.lambda[c] = o.v[7];
        a.d.dPpsi[c] = o.v[8];
        a.d.P_num[c] = a.d.gamma_eff[c] * a.f.RP[c] + o.v[8];      // θc = γ_eff RP + ΔPψ
        if (!LIN) {
            const double T = (vfields && a.f.T) ? (a.tg ? a.f.T[(i + 1) + (nx + 2) * (j + 1)] : a.f.T[c]) : 0.0;      // local_viscosity_args: T[I .+ 1]
            a.f.eta[c] = dy_visc<3>(a.rh, a.nu, a.cut_lo, a.cut_hi, rc, o.v, T, Pc, eta);
        }
    }
}

// the momentum residuals d_xa(τxx) + d_yi(τxy) - d_xa(P) - d_xa(θ) - av_xa(ρgx) and the y analogue (MiniKernels.jl:37-72), θ = ΔPψ (PH) or θc (DR)
struct DyMom { const double *P, *th, *txx, *tyy, *txy, *fx, *fy; double _dx, _dy; int nx, ny; };
__device__ __forceinline__ double dy_Rx(const DyMom &m, const int i, const int j)
{
    const int nx = m.nx, c = i + nx * j;
    return (-m.txx[c] + m.txx[c + 1]) * m._dx + (-V2(m.txy, i + 1, j) + V2(m.txy, i + 1, j + 1)) * m._dy - (-m.P[c] + m.P[c + 1]) * m._dx -
           (-m.th[c] + m.th[c + 1]) * m._dx - (m.fx[c] + m.fx[c + 1]) * 0.5;
}
__device__ __forceinline__ double dy_Ry(const DyMom &m, const int i, const int j)
{
    const int nx = m.nx, c = i + nx * j;
    return (-m.tyy[c] + m.tyy[c + nx]) * m._dy + (-V2(m.txy, i, j + 1) + V2(m.txy, i + 1, j + 1)) * m._dx - (-m.P[c] + m.P[c + nx]) * m._dy -
           (-m.th[c] + m.th[c + nx]) * m._dy - (m.fy[c] + m.fy[c + nx]) * 0.5;
}

// compute_PH_residual_V! (velocity_kernels.jl:326-349)
__global__ __launch_bounds__(256) void k_dy_ph_residual(const DyMom m, double *__restrict__ Rx, double *__restrict__ Ry)
{
    const int nx = m.nx;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= m.ny) return;
    if (i < nx - 1) Rx[i + (nx - 1) * j] = dy_Rx(m, i, j);
    if (j < m.ny - 1) Ry[t] = dy_Ry(m, i, j);
}

// compute_DR_residual_update_V! (velocity_kernels.jl:671-727).  BCF: the thread that moves a velocity node next to a free-slip / no-slip face refreshes that
// node's ghost copy, as velocity2d_cell does (stokes2d_kernels.hpp): all flow_bcs! changes once it has been applied in full one time
struct DyUpd { double *Rx, *Ry, *Vx, *Vy, *dVxdtau, *dVydtau; const double *Dx, *Dy, *ax, *ay, *bx, *by, *tx, *ty; unsigned fs, ns; };
template <bool BCF>
__global__ __launch_bounds__(256) void k_dy_update(const DyMom m, const DyUpd u)
{
    const int nx = m.nx, ny = m.ny;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    if (i < nx - 1) {
        const int k = i + (nx - 1) * j, q = (i + 1) + (nx + 1) * (j + 1);
        const double R = dy_Rx(m, i, j) / u.Dx[k];
        u.Rx[k] = R;
        const double dnew = u.ax[k] * u.dVxdtau[k] + R;      // damped_update_V :660-663
        u.dVxdtau[k] = dnew;
        const double v = u.Vx[q] + dnew * u.bx[k] * u.tx[k];
        u.Vx[q] = v;
        if (BCF) {
            if (j == 0) { if (u.fs & JRX_FACE_BOT) u.Vx[q - (nx + 1)] = v; else if (u.ns & JRX_FACE_BOT) u.Vx[q - (nx + 1)] = -v; }
            if (j == ny - 1) { if (u.fs & JRX_FACE_TOP) u.Vx[q + (nx + 1)] = v; else if (u.ns & JRX_FACE_TOP) u.Vx[q + (nx + 1)] = -v; }
        }
    }
    if (j < ny - 1) {
        const int q = (i + 1) + (nx + 2) * (j + 1);
        const double R = dy_Ry(m, i, j) / u.Dy[t];
        u.Ry[t] = R;
        const double dnew = u.ay[t] * u.dVydtau[t] + R;
        u.dVydtau[t] = dnew;
        const double v = u.Vy[q] + dnew * u.by[t] * u.ty[t];
        u.Vy[q] = v;
        if (BCF) {
            if (i == 0) { if (u.fs & JRX_FACE_LEFT) u.Vy[q - 1] = v; else if (u.ns & JRX_FACE_LEFT) u.Vy[q - 1] = -v; }
            if (i == nx - 1) { if (u.fs & JRX_FACE_RIGHT) u.Vy[q + 1] = v; else if (u.ns & JRX_FACE_RIGHT) u.Vy[q + 1] = -v; }
        }
    }
}

// _Gershgorin_Stokes2D_SchurComplement! (Gershgorin.jl:21-155), uniform spacing: _dx = inv(dx), _dy = inv(dy)
__global__ __launch_bounds__(256) void k_dy_gershgorin(const DyArgs a)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / nx, i = t - j * nx;
    if (j >= ny) return;
    const double *__restrict__ eta = a.f.eta, *__restrict__ etav = a.f.eta_v, *__restrict__ gam = a.d.gamma_eff;
    const double dt = a.dt, _dx = a._dx, _dy = a._dy;
    const double _dx2 = _dx * _dx, _dy2 = _dy * _dy, _dxdy = _dx * _dy, c43 = 4.0 / 3.0, c23 = 2.0 / 3.0;
#define GV(i_, j_) ratio_avg(a.rh.G, a.f.phase_v + np * ((i_) + (nx + 1) * (j_)), np)
#define GC(i_, j_) ratio_avg(a.rh.G, a.f.phase_c + np * ((i_) + nx * (j_)), np)
#define VE(e_, G_) (1 / (1 / (e_) + 1 / ((G_) * dt)))
    const double Gne = GV(i + 1, j + 1), Gc = GC(i, j);
    const double e_c = eta[t], g_c = gam[t], e_ne = V2(etav, i + 1, j + 1);
    if (i < nx - 1) {
        const double gE = gam[t + 1], gW = g_c;
        const double eN = VE(e_ne, Gne), eS = VE(V2(etav, i + 1, j), GV(i + 1, j)), eW = VE(e_c, Gc), eE = VE(eta[t + 1], GC(i + 1, j));
        const double eN_dy = eN * _dy, eS_dy = eS * _dy, eE_dx = eE * _dx, eW_dx = eW * _dx, gE_dx = gE * _dx, gW_dx = gW * _dx;
        const double D = (eN_dy + eS_dy) * _dy + (gE_dx + gW_dx + c43 * (eE_dx + eW_dx)) * _dx;
        const double Cxx = fabs(eN * _dy2) + fabs(eS * _dy2) + fabs((gE + c43 * eE) * _dx2) + fabs((gW + c43 * eW) * _dx2) + fabs(D);
        const double Cxy = fabs((gE - c23 * eE + eN) * _dxdy) + fabs((gE - c23 * eE + eS) * _dxdy) + fabs((gW + eN - c23 * eW) * _dxdy) +
                           fabs((gW + eS - c23 * eW) * _dxdy);
        const int k = i + (nx - 1) * j;
        a.d.Dx[k] = D;
        a.d.lmaxVx[k] = (1 / D) * (Cxx + Cxy);
    }
    if (j < ny - 1) {
        const double gN = gam[t + nx], gS = g_c;
        const double eN = VE(eta[t + nx], GC(i, j + 1)), eS = VE(e_c, Gc), eW = VE(V2(etav, i, j + 1), GV(i, j + 1)), eE = VE(e_ne, Gne);
        const double eE_dx = eE * _dx, eW_dx = eW * _dx, eN_dy = eN * _dy, eS_dy = eS * _dy, gN_dy = gN * _dy, gS_dy = gS * _dy;
        const double D = (gN_dy + gS_dy + c43 * (eN_dy + eS_dy)) * _dy + (eE_dx + eW_dx) * _dx;
        const double Cyy = fabs(eE * _dx2) + fabs(eW * _dx2) + fabs((gN + c43 * eN) * _dy2) + fabs((gS + c43 * eS) * _dy2) + fabs(D);
        const double Cyx = fabs((gN + eE - c23 * eN) * _dxdy) + fabs((gN - c23 * eN + eW) * _dxdy) + fabs((gS + eE - c23 * eS) * _dxdy) +
                           fabs((gS - c23 * eS + eW) * _dxdy);
        a.d.Dy[t] = D;
        a.d.lmaxVy[t] = (1 / D) * (Cyx + Cyy);
    }
#undef GV
#undef GC
#undef VE
}

// the epilogue (solver.jl:269-286): P += ΔPψ, compute_∇V!, compute_vorticity!, shear2center! of ε, ε_pl, Δε, accumulate_tensor!, accumulate_vol!
__global__ __launch_bounds__(256) void k_dy_epilogue(const DyArgs a)
{
    const int nx = a.nx, ny = a.ny;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy;
    if (a.f.omega_xy)
        a.f.omega_xy[t] = 0.5 * ((-Vy[i + (nx + 2) * j] + Vy[(i + 1) + (nx + 2) * j]) * a._dx - (-Vx[i + (nx + 1) * j] + Vx[i + (nx + 1) * (j + 1)]) * a._dy);
    if (i < nx && j < ny) {
        const int c = i + nx * j;
        a.f.P[c] = a.f.P[c] + a.d.dPpsi[c];
        a.f.divV[c] = (-Vx[i + (nx + 1) * (j + 1)] + Vx[(i + 1) + (nx + 1) * (j + 1)]) * a._dx + (-Vy[(i + 1) + (nx + 2) * j] + Vy[(i + 1) + (nx + 2) * (j + 1)]) * a._dy;
#define S2C(V) (0.25 * (V2(V, i, j) + V2(V, i + 1, j) + V2(V, i, j + 1) + V2(V, i + 1, j + 1)))
        if (a.f.exy_c) a.f.exy_c[c] = S2C(a.f.exy);
        if (a.f.eplxy_c) a.f.eplxy_c[c] = S2C(a.f.eplxy);
        if (a.f.dexy_c && a.f.dexy) a.f.dexy_c[c] = S2C(a.f.dexy);
#undef S2C
        const double p = V2(a.f.eplxy, i, j), q = V2(a.f.eplxy, i + 1, j), r = V2(a.f.eplxy, i, j + 1), s = V2(a.f.eplxy, i + 1, j + 1);
        const double xx = a.f.eplxx[c], yy = a.f.eplyy[c];
        a.f.EII_pl[c] += sqrt(0.5 * (xx * xx + yy * yy) + 0.25 * (p * p + q * q + r * r + s * s)) * a.dt;
        a.f.EVol_pl[c] += a.dt * a.f.evol_pl[c];
    }
}
#undef C2
#undef V2

// what every DYREL entry point refuses (status JRX_ERR_ARG, each named), before anything is launched
jrx_status dy_check(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                    const jrx_vep2d_params *p)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !d || !p) return jrx_fail(h, JRX_ERR_ARG, "DYREL: null argument");
    JRX_TRY(jrx_check_device(h));
    if (jrx_comm_active(h)) return jrx_fail(h, JRX_ERR_ARG, "DYREL: a communicator of more than one rank is not built (single block only)");
    for (int q = 0; q < 6; q++)
        if (p->inv_spacing[q]) return jrx_fail(h, JRX_ERR_ARG, "DYREL: a non-uniform Geometry (inv_spacing) is not built");
    if (phi) return jrx_fail(h, JRX_ERR_ARG, "DYREL: the variational form with a RockRatio is not built");
    if (d->dT) return jrx_fail(h, JRX_ERR_ARG, "DYREL: the thermal form of the pressure residual (args.ΔT) is not built");
    if (d->melt_fraction) return jrx_fail(h, JRX_ERR_ARG, "DYREL: the melt-fraction form of the pressure residual (args.melt_fraction) is not built");
    if (p->periodic) return jrx_fail(h, JRX_ERR_ARG, "DYREL: periodic velocity boundary conditions are not built");
    if (p->nx < 3 || p->ny < 3) return jrx_fail(h, JRX_ERR_ARG, "DYREL: needs at least 3 cells per dimension");
    if (rh) {
        if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
        for (int q = 0; q < rh->nphase; q++)
            if (rh->is_pl[q] != 0 && rh->is_pl[q] != 1) return jrx_fail(h, JRX_ERR_ARG, "DYREL: is_pl = %d of phase %d is not built (0 or 1: none, DruckerPrager_regularised)", (int)rh->is_pl[q], q);
    }
    if ((p->nx + 2) * (p->ny + 2) * (int64_t)(rh ? rh->nphase : 1) >= (int64_t)1 << 31)
        return jrx_fail(h, JRX_ERR_ARG, "DYREL: an array of 2^31 or more entries exceeds the 32-bit offsets of its kernels");
    return JRX_OK;
}

// the launches of this file's kernels on the handle's stream: what the entry points below call, and the launch object of dy_solve (dyrel_common.hpp)
struct Dy2 {
    typedef DyArgs Args;
    static constexpr int ND = 2, MAXBLK = 1024;      // partial rows of 8: half of kMaxRedBlocks rows of 4
    jrx_handle *h;
    hipStream_t s;
    DyArgs a;
    double dofs[2], pdof;      // velocity_dofs(Val(2)), pressure_dof (solver.jl:349-357)
    bool bcs_applied = false;      // flow_bcs! has run in full on V since the solve began

    Dy2(jrx_handle *h_, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh, const jrx_vep2d_params *p) : h(h_), s(h_->stream)
    {
        memset(&a, 0, sizeof(a));
        a.f = *f; a.d = *d;
        if (rh) a.rh = *rh;
        a._dx = p->_dx; a._dy = p->_dy; a.dt = p->dt;
        a.nx = (int)p->nx; a.ny = (int)p->ny;
        a.fs = p->free_slip; a.ns = p->no_slip;
        a.tg = p->T_ghosted != 0;
        a.rel = 1.0; a.nu = 1.0e-2; a.cut_lo = -INFINITY; a.cut_hi = INFINITY;
        dofs[0] = (double)((p->nxg - 2) * (p->nyg - 1)); dofs[1] = (double)((p->nxg - 1) * (p->nyg - 2));
        pdof = (double)(p->nxg * p->nyg);
    }
    int cells() const { return a.nx * a.ny; }
    dim3 gv() const { return dim3(dy_g1((a.nx + 1) * (a.ny + 1))); }
    dim3 gc() const { return dim3(dy_g1(cells())); }
    DyMom mom(const double *th) const { return DyMom{a.f.P, th, a.f.txx, a.f.tyy, a.f.txy, a.f.fx, a.f.fy, a._dx, a._dy, a.nx, a.ny}; }
    DyUpd upd() const
    {
        const jrx_dyrel2d_fields &d = a.d;
        return DyUpd{a.f.Rx, a.f.Ry, a.f.Vx, a.f.Vy, d.dVxdtau, d.dVydtau, d.Dx, d.Dy, d.alphaVx, d.alphaVy, d.betaVx, d.betaVy, d.dtauVx, d.dtauVy, a.fs, a.ns};
    }
    DyDof<2> dof() const
    {
        const jrx_dyrel2d_fields &d = a.d;
        const int nxn = (a.nx - 1) * a.ny, nyn = a.nx * (a.ny - 1);
        return DyDof<2>{{a.f.Rx, a.f.Ry}, {d.Rx0, d.Ry0}, {d.Dx, d.Dy}, {d.lmaxVx, d.lmaxVy}, {d.dVxdtau, d.dVydtau}, {d.dtauVx, d.dtauVy}, {d.dVx, d.dVy},
                        {d.betaVx, d.betaVy}, {d.cVx, d.cVy}, {d.alphaVx, d.alphaVy}, {nxn, nyn}, nxn > nyn ? nxn : nyn};
    }

    jrx_status strain_rp(bool strain) const
    {
        if (strain) hipLaunchKernelGGL(k_dy_strain_rp<true>, gv(), dim3(256), 0, s, a.f.exx, a.f.eyy, a.f.exy, (const double *)a.f.Vx, (const double *)a.f.Vy,
                                       a.f.RP, (const double *)a.f.P, (const double *)a.f.P0, (const double *)a.f.Q, (const double *)a.d.etab, a._dx, a._dy, a.dt, a.nx, a.ny);
        else hipLaunchKernelGGL(k_dy_strain_rp<false>, gv(), dim3(256), 0, s, a.f.exx, a.f.eyy, a.f.exy, (const double *)a.f.Vx, (const double *)a.f.Vy,
                                a.f.RP, (const double *)a.f.P, (const double *)a.f.P0, (const double *)a.f.Q, (const double *)a.d.etab, a._dx, a._dy, a.dt, a.nx, a.ny);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status stress(bool lin) const
    {
        const bool soft = mat_has_softening(&a.rh);
        if (soft) {
            if (lin) hipLaunchKernelGGL((k_dy_stress<true, true>), gv(), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_dy_stress<true, false>), gv(), dim3(256), 0, s, a);
        } else {
            if (lin) hipLaunchKernelGGL((k_dy_stress<false, true>), gv(), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_dy_stress<false, false>), gv(), dim3(256), 0, s, a);
        }
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status ph_residual() const
    {
        hipLaunchKernelGGL(k_dy_ph_residual, gc(), dim3(256), 0, s, mom(a.d.dPpsi), a.f.Rx, a.f.Ry);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status copy_old_residual() const
    {
        const DyDof<2> q = dof();
        hipLaunchKernelGGL(k_copy6, dim3(256), dim3(256), 0, s, q.R0[0], (const double *)q.R[0], (i64)q.n[0], q.R0[1], (const double *)q.R[1], (i64)q.n[1],
                           (double *)nullptr, (const double *)nullptr, (i64)0, (double *)nullptr, (const double *)nullptr, (i64)0, (double *)nullptr,
                           (const double *)nullptr, (i64)0, (double *)nullptr, (const double *)nullptr, (i64)0);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    // BCF: flow_bcs! in full the first time; afterwards the update kernel refreshes the ghosts of the nodes it moves
    jrx_status update(bool BCF) const
    {
        if (BCF) hipLaunchKernelGGL(k_dy_update<true>, gc(), dim3(256), 0, s, mom(a.d.P_num), upd());
        else hipLaunchKernelGGL(k_dy_update<false>, gc(), dim3(256), 0, s, mom(a.d.P_num), upd());
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status update_V(bool, bool)
    {
        JRX_TRY(update(bcs_applied));
        if (!bcs_applied) { JRX_TRY(jrx2d_bcs(h, s, a.f.Vx, a.f.Vy, a.nx, a.ny, a.fs, a.ns, 0)); bcs_applied = true; }
        return JRX_OK;
    }
    jrx_status gershgorin() const
    {
        hipLaunchKernelGGL(k_dy_gershgorin, gc(), dim3(256), 0, s, a);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status rhog() const      // ρg[end] = ρg y
    {
        const int64_t nn[3] = {a.nx, a.ny, 1}, tdim[3] = {a.tg ? a.nx + 2 : a.nx, a.tg ? a.ny + 2 : a.ny, 1};
        return jrx_compute_rhog(h, a.f.fy, &a.rh, a.f.phase_c, a.f.T, a.f.P, nn, tdim, 2);
    }
    jrx_status epilogue() const
    {
        const i64 n = cells(), nv = (i64)(a.nx + 1) * (a.ny + 1);
        hipLaunchKernelGGL(k_dy_epilogue, gv(), dim3(256), 0, s, a);
        DY_LAUNCH(h);
        hipLaunchKernelGGL(k_copy6, dim3(256), dim3(256), 0, s, a.f.toxx, (const double *)a.f.txx, n, a.f.toyy, (const double *)a.f.tyy, n, a.f.toxy,
                           (const double *)a.f.txy, nv, a.f.toxy_c, (const double *)a.f.txy_c, n, a.d.toxx_v, (const double *)a.d.txx_v, nv, a.d.toyy_v,
                           (const double *)a.d.tyy_v, nv);
        DY_LAUNCH(h);
        return JRX_OK;
    }
};

#define DY_FIELDS_STRESS(f, d)                                                                                                                                  \
    (f)->P, (f)->exx, (f)->eyy, (f)->exy, (f)->eplxx, (f)->eplyy, (f)->eplxy, (f)->txx, (f)->tyy, (f)->txy, (f)->txy_c, (f)->tII, (f)->toxx, (f)->toyy, (f)->toxy,  \
        (f)->toxy_c, (f)->eta, (f)->eta_v, (f)->eta_vep, (f)->EII_pl, (f)->evol_pl, (f)->RP, (f)->phase_c, (f)->phase_v, (d)->txx_v, (d)->tyy_v, (d)->toxx_v,       \
        (d)->toyy_v, (d)->lambda, (d)->lambda_v, (d)->dPpsi, (d)->P_num, (d)->gamma_eff
#define DY_FIELDS_MOM(f) (f)->P, (f)->txx, (f)->tyy, (f)->txy, (f)->fx, (f)->fy, (f)->Rx, (f)->Ry
#define DY_FIELDS_DAMP(d)                                                                                                                                      \
    (d)->Dx, (d)->Dy, (d)->lmaxVx, (d)->lmaxVy, (d)->dVxdtau, (d)->dVydtau, (d)->dtauVx, (d)->dtauVy, (d)->dVx, (d)->dVy, (d)->betaVx, (d)->betaVy, (d)->cVx,      \
        (d)->cVy, (d)->alphaVx, (d)->alphaVy, (d)->Rx0, (d)->Ry0

}   // namespace

extern "C" {

jrx_status jrx_dyrel2d_strain_rate_RP(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p, int32_t do_strain_rate)
{
    JRX_TRY(dy_check(h, f, d, nullptr, nullptr, p));
    DY_REQ(h, "compute_∇V_strain_rate_RP!", f->exx, f->eyy, f->exy, f->Vx, f->Vy, f->RP, f->P, f->P0, f->Q, d->etab);
    JRX_TRY(Dy2(h, f, d, nullptr, p).strain_rp(do_strain_rate != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_stress_viscosity(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh, const jrx_vep2d_params *p,
                                        const jrx_dyrel2d_params *dp, double lambda_relaxation)
{
    JRX_TRY(dy_check(h, f, d, nullptr, rh, p));
    if (!rh || !dp) return jrx_fail(h, JRX_ERR_ARG, "DYREL: null argument");
    DY_REQ(h, "compute_stress_viscosity_DRYEL!", DY_FIELDS_STRESS(f, d));
    Dy2 o(h, f, d, rh, p);
    o.a.rel = lambda_relaxation; o.a.nu = dp->viscosity_relaxation; o.a.cut_lo = dp->cutoff_lo; o.a.cut_hi = dp->cutoff_hi;
    JRX_TRY(o.stress(dp->linear_viscosity != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_PH_residual(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p)
{
    JRX_TRY(dy_check(h, f, d, nullptr, nullptr, p));
    DY_REQ(h, "compute_PH_residual_V!", DY_FIELDS_MOM(f), d->dPpsi);
    JRX_TRY(Dy2(h, f, d, nullptr, p).ph_residual());
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_DR_residual_update_V(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p)
{
    JRX_TRY(dy_check(h, f, d, nullptr, nullptr, p));
    DY_REQ(h, "compute_DR_residual_update_V!", DY_FIELDS_MOM(f), f->Vx, f->Vy, d->P_num, d->Dx, d->Dy, d->dVxdtau, d->dVydtau, d->alphaVx, d->alphaVy, d->betaVx,
           d->betaVy, d->dtauVx, d->dtauVy);
    JRX_TRY(Dy2(h, f, d, nullptr, p).update(false));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_gershgorin(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh, const jrx_vep2d_params *p)
{
    JRX_TRY(dy_check(h, f, d, nullptr, rh, p));
    if (!rh) return jrx_fail(h, JRX_ERR_ARG, "DYREL: null argument");
    DY_REQ(h, "Gershgorin_Stokes2D_SchurComplement!", f->eta, f->eta_v, f->phase_c, f->phase_v, d->gamma_eff, d->Dx, d->Dy, d->lmaxVx, d->lmaxVy);
    JRX_TRY(Dy2(h, f, d, rh, p).gershgorin());
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_update_dtauV_alpha_beta(jrx_handle *h, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p, double CFL, int32_t from_lambda_max)
{
    jrx_vep2d_fields none;
    memset(&none, 0, sizeof(none));
    JRX_TRY(dy_check(h, &none, d, nullptr, nullptr, p));
    DY_REQ(h, "update_dτV_α_β!", d->dtauVx, d->dtauVy, d->betaVx, d->betaVy, d->alphaVx, d->alphaVy, d->cVx, d->cVy, d->lmaxVx, d->lmaxVy);
    JRX_TRY(dy_dtau(Dy2(h, &none, d, nullptr, p), CFL, from_lambda_max != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_bulk_viscosity_and_penalty(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh,
                                                  const jrx_vep2d_params *p, double gamma_fact)
{
    JRX_TRY(dy_check(h, f, d, nullptr, rh, p));
    if (!rh) return jrx_fail(h, JRX_ERR_ARG, "DYREL: null argument");
    DY_REQ(h, "compute_bulk_viscosity_and_penalty!", f->eta, f->phase_c, d->etab, d->gamma_eff);
    JRX_TRY(dy_bulk(Dy2(h, f, d, rh, p), gamma_fact));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_init(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                            const jrx_vep2d_params *p, const jrx_dyrel2d_params *dp)
{
    JRX_TRY(dy_check(h, f, d, phi, rh, p));
    if (!rh || !dp) return jrx_fail(h, JRX_ERR_ARG, "DYREL: null argument");
    DY_REQ(h, "DYREL!", f->eta, f->eta_v, f->phase_c, f->phase_v, d->gamma_eff, d->etab, DY_FIELDS_DAMP(d));
    JRX_TRY(dy_init(Dy2(h, f, d, rh, p), dp->CFL, dp->gamma_fact));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel2d_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                             const jrx_vep2d_params *p, const jrx_dyrel2d_params *dp, jrx_dyrel2d_result *res)
{
    JRX_TRY(dy_check(h, f, d, phi, rh, p));
    if (!rh || !dp || !res) return jrx_fail(h, JRX_ERR_ARG, "DYREL: null argument");
    if (dp->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    DY_REQ(h, "solve_DYREL!", DY_FIELDS_STRESS(f, d), DY_FIELDS_MOM(f), DY_FIELDS_DAMP(d), f->P0, f->divV, f->Q, f->Vx, f->Vy, f->eplxy_c, f->EVol_pl, d->etab);
    if (mat_viscosity_reads_invariant(rh) && !f->exy_c) return jrx_fail(h, JRX_ERR_ARG, "a power-law creep needs ε.xy_c for compute_viscosity!");
    Dy2 o(h, f, d, rh, p);
    o.a.nu = dp->viscosity_relaxation; o.a.cut_lo = dp->cutoff_lo; o.a.cut_hi = dp->cutoff_hi;
    hipStream_t s = o.s;
    const size_t n = (size_t)o.cells(), nv = (size_t)(o.a.nx + 1) * (o.a.ny + 1);

    // solver.jl:86-95: P0 <- P, @tensor_center(ε_pl) = 0, λ = λv = 0
    JRX_HIP(h, hipMemcpyAsync(f->P0, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    JRX_HIP(h, hipMemsetAsync(f->eplxx, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplyy, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(f->eplxy_c, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_v, 0, nv * sizeof(double), s));
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    {   // :117: compute_viscosity! (relaxation 1, the strain-rate invariant)
        jrx_vep2d_params pv = *p;
        pv.cutoff_lo = dp->cutoff_lo; pv.cutoff_hi = dp->cutoff_hi;
        JRX_TRY(jrx_vep2d_compute_viscosity(h, f, rh, &pv, 1.0));
    }
    return dy_solve(o, dp, res);
}

}   // extern "C"
