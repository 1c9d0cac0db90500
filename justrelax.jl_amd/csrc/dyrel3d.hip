// dyrel3d.hip -- 3D DYREL (self-tuned dynamic relaxation inside Powell-Hestenes pressure iterations) for gfx950: kernels, per-kernel entry points, driver.
//
// Reference (PTsolvers/JustRelax.jl).  Restated: src/DYREL/constructors.jl:61-111 (the 3D allocator), :178-190 (DYREL!), :230-254 (compute_bulk_viscosity_and_penalty!),
// solver.jl:44-294 (_solve_DYREL!), :329-365 (dyrel_fields(Val(3)), velocity_dofs, pressure_dof, compute_λminV!), velocity_kernels.jl:242-322
// (compute_∇V_strain_rate_RP! 3D), :441-477 (compute_PH_residual_V! 3D), :625-663 (compute_dV!, update_cV!, damped_update_V), :729-828 (compute_DR_residual_update_V! 3D),
// Gershgorin.jl:171-310 (update_α_β!, update_dτV_α_β!), stress_kernels.jl:224-315 (the local law, dyrel_local.hpp).
// No reference text (the reference cannot run a 3D solve): the stress kernel and the eigenvalue bound; their forms are stated in include/jrx.h and below.
//
// Departures.  (1) The reference's 3D momentum residuals take d_yi / d_zi / d_xi of the shear stresses from MiniKernels.jl:53-55, which read A[i+1, j+1, k+1]: one plane
// past τxy and across two planes elsewhere.  Built instead: the index triples of the unmasked 3D velocity kernel (src/stokes/VelocityKernels.jl:215-238), the
// 2D DYREL residual one dimension up, in the reference's term order (normal, shear, shear, -∇P, -∇θ, -ρg).  (2) No vertex-normal stresses (τ.xx_v ...), no ηv.
// (3) The τII viscosity refresh happens at the centres only; an edge takes harm_clamped(η).
//
// An inner iteration: k_dy3_strain_rp -> k_dy3_stress (edges) -> k_dy3_stress (centres) -> k_dy3_update -> flow_bcs!.  The stress kernel is two launches: the centre
// half rewrites η (unless linear_viscosity), which the edge half of the neighbouring nodes reads through harm_clamped; edges first, then centres, so every edge sees
// the η of the previous refresh whatever the schedule.  Everything else the stress kernel writes is read by the same launch at the thread's own index only; the
// edges average τ_o, ε, P, EII_pl, which it never writes.  32-bit element offsets (the extents are checked against 2^31).  fma only in update_α_β (the reference's @muladd).
#include <initializer_list>
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_material.hpp"
#include "dyrel_local.hpp"
#include "edge_stencils3d.hpp"

namespace {

struct Dy3Args {
    jrx_vep3d_fields f;
    jrx_dyrel3d_fields d;
    jrx_rheology rh;
    double _dx, _dy, _dz, dt, rel, nu, cut_lo, cut_hi;
    int nx, ny, nz;
    unsigned fs, ns;
    bool tg;
};

// node (i, j, k) of an (n1, n2, n3) box: block = 64 nodes in x, 4 in y; k = blockIdx.z.  x fastest across the wave.
#define DY3_NODE(n1_, n2_)                                                                   \
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6), k = blockIdx.z; \
    if (i >= (n1_) || j >= (n2_)) return;
#define DY3_GRID(n1_, n2_, n3_) dim3((unsigned)(((n1_) + 63) / 64), (unsigned)(((n2_) + 3) / 4), (unsigned)(n3_))
#define C3(A, i_, j_, k_) (A)[(i_) + nx * ((j_) + ny * (k_))]
#define EYZ(A, i_, j_, k_) (A)[(i_) + nx * ((j_) + (ny + 1) * (k_))]
#define EXZ(A, i_, j_, k_) (A)[(i_) + (nx + 1) * ((j_) + ny * (k_))]
#define EXY(A, i_, j_, k_) (A)[(i_) + (nx + 1) * ((j_) + (ny + 1) * (k_))]
#define VX(i_, j_, k_) Vx[(i_) + (nx + 1) * ((j_) + (ny + 2) * (k_))]
#define VY(i_, j_, k_) Vy[(i_) + (nx + 2) * ((j_) + (ny + 1) * (k_))]
#define VZ(i_, j_, k_) Vz[(i_) + (nx + 2) * ((j_) + (ny + 2) * (k_))]

// compute_∇V_strain_rate_RP! 3D (velocity_kernels.jl:242-322): one thread per node of ni .+ 1; ∇V stays in a register
template <bool STRAIN>
__global__ __launch_bounds__(256) void k_dy3_strain_rp(double *__restrict__ exx, double *__restrict__ eyy, double *__restrict__ ezz, double *__restrict__ eyz,
                                                       double *__restrict__ exz, double *__restrict__ exy, const double *__restrict__ Vx, const double *__restrict__ Vy,
                                                       const double *__restrict__ Vz, double *__restrict__ RP, const double *__restrict__ P, const double *__restrict__ P0,
                                                       const double *__restrict__ Q, const double *__restrict__ etab, const double _dx, const double _dy, const double _dz,
                                                       const double dt, const int nx, const int ny, const int nz)
{
    DY3_NODE(nx + 1, ny + 1)
    if (i < nx && j < ny && k < nz) {
        const int c = i + nx * (j + ny * k);
        const double dVx_dx = (VX(i + 1, j + 1, k + 1) - VX(i, j + 1, k + 1)) * _dx;
        const double dVy_dy = (VY(i + 1, j + 1, k + 1) - VY(i + 1, j, k + 1)) * _dy;
        const double dVz_dz = (VZ(i + 1, j + 1, k + 1) - VZ(i + 1, j + 1, k)) * _dz;
        const double div = dVx_dx + dVy_dy + dVz_dz;
        if (STRAIN) {
            const double div_third = div * (1.0 / 3.0);
            exx[c] = dVx_dx - div_third;
            eyy[c] = dVy_dy - div_third;
            ezz[c] = dVz_dz - div_third;
        }
        RP[c] = -div - (P[c] - P0[c]) / etab[c] + (Q[c] / dt);      // _compute_RP!, pressure_kernels.jl:112
    }
    if (STRAIN) {
        if (i < nx) EYZ(eyz, i, j, k) = 0.5 * (_dz * (VY(i + 1, j, k + 1) - VY(i + 1, j, k)) + _dy * (VZ(i + 1, j + 1, k) - VZ(i + 1, j, k)));
        if (j < ny) EXZ(exz, i, j, k) = 0.5 * (_dz * (VX(i, j + 1, k + 1) - VX(i, j + 1, k)) + _dx * (VZ(i + 1, j + 1, k) - VZ(i, j + 1, k)));
        if (k < nz) EXY(exy, i, j, k) = 0.5 * (_dy * (VX(i, j + 1, k + 1) - VX(i, j, k + 1)) + _dx * (VY(i + 1, j, k + 1) - VY(i, j, k + 1)));
    }
}

// one edge of family T (0 yz, 1 xz, 2 xy) inside its array: the gathers of update_stresses_center_vertex_ps! 3D (src/stokes/StressKernels.jl:705-733 and its
// siblings), then the local law with 6 components; keeps the edge's own shear stress, its plastic shear strain rate and its λv
template <int T, bool SOFT>
__device__ __forceinline__ void dy3_edge_at(const Dy3Args &a, const int i, const int j, const int k, const int ci[3], const int cj[3], const int ck[3])
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const int n1 = nx + (T != 0), n2 = ny + (T != 1);
    const int v = i + n1 * (j + n2 * k);
    int oc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) oc[q] = ci[cen3(T, q, 0)] + nx * (cj[cen3(T, q, 1)] + ny * ck[cen3(T, q, 2)]);
#define AVC(A) (0.25 * ((A)[oc[0]] + (A)[oc[1]] + (A)[oc[2]] + (A)[oc[3]]))
    const double etav = 4 / (1 / a.f.eta[oc[0]] + 1 / a.f.eta[oc[1]] + 1 / a.f.eta[oc[2]] + 1 / a.f.eta[oc[3]]);      // harm_clamped_*
    const double Pv = AVC(a.f.P);
    const double EIIv = AVC(a.f.EII_pl);
    double eij[6] = {AVC(a.f.exx), AVC(a.f.eyy), AVC(a.f.ezz), 0, 0, 0};
    double toij[6] = {AVC(a.f.toxx), AVC(a.f.toyy), AVC(a.f.tozz), 0, 0, 0};
#undef AVC
    const double *const esh[3] = {a.f.eyz, a.f.exz, a.f.exy}, *const tosh[3] = {a.f.toyz, a.f.toxz, a.f.toxy};
#pragma unroll
    for (int s = 0; s < 3; s++) {
        if (s == T) { eij[3 + s] = esh[s][v]; toij[3 + s] = tosh[s][v]; continue; }
        const int m1 = nx + (s != 0), m2 = ny + (s != 1);
        int o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = ci[oth3(T, s, q, 0)] + m1 * (cj[oth3(T, s, q, 1)] + m2 * ck[oth3(T, s, q, 2)]);
        eij[3 + s] = 0.25 * (esh[s][o[0]] + esh[s][o[1]] + esh[s][o[2]] + esh[s][o[3]]);
        toij[3 + s] = 0.25 * (tosh[s][o[0]] + tosh[s][o[1]] + tosh[s][o[2]] + tosh[s][o[3]]);
    }
    const double *const phsh[3] = {a.f.phase_yz, a.f.phase_xz, a.f.phase_xy};
    double *const tsh[3] = {a.f.tyz, a.f.txz, a.f.txy}, *const eplsh[3] = {a.f.eplyz, a.f.eplxz, a.f.eplxy};
    double *const lamv[3] = {a.d.lambda_yz, a.d.lambda_xz, a.d.lambda_xy};
    typedef DyLocal<6> L;
    const L o = dy_local_stress<SOFT, 6>(a.rh, phsh[T] + np * v, eij, toij, etav, Pv, lamv[T][v], a.rel, a.dt, EIIv);
    tsh[T][v] = o.v[3 + T];
    eplsh[T][v] = o.v[6 + 3 + T];
    lamv[T][v] = o.v[L::LAM];
}

// the centre (i, j, k): compute_stress_viscosity_DRYEL!'s centre half (stress_kernels.jl:186-218) with 6 components
template <bool SOFT, bool LIN>
__device__ __forceinline__ void dy3_centre_at(const Dy3Args &a, const int i, const int j, const int k)
{
    const int nx = a.nx, ny = a.ny, np = a.rh.nphase;
    const int c = i + nx * (j + ny * k);
    double eij[6] = {a.f.exx[c], a.f.eyy[c], a.f.ezz[c], 0, 0, 0};
    // sum(_gather(A)) / 4 of each edge family, the summation order of the 2D text: k outer, j, i inner
    eij[3] = (EYZ(a.f.eyz, i, j, k) + EYZ(a.f.eyz, i, j + 1, k) + EYZ(a.f.eyz, i, j, k + 1) + EYZ(a.f.eyz, i, j + 1, k + 1)) / 4;
    eij[4] = (EXZ(a.f.exz, i, j, k) + EXZ(a.f.exz, i + 1, j, k) + EXZ(a.f.exz, i, j, k + 1) + EXZ(a.f.exz, i + 1, j, k + 1)) / 4;
    eij[5] = (EXY(a.f.exy, i, j, k) + EXY(a.f.exy, i + 1, j, k) + EXY(a.f.exy, i, j + 1, k) + EXY(a.f.exy, i + 1, j + 1, k)) / 4;
    const double toij[6] = {a.f.toxx[c], a.f.toyy[c], a.f.tozz[c], a.f.toyz_c[c], a.f.toxz_c[c], a.f.toxy_c[c]};
    const double eta = a.f.eta[c], Pc = a.f.P[c];
    const double *rc = a.f.phase_c + np * c;
    typedef DyLocal<6> L;
    const L o = dy_local_stress<SOFT, 6>(a.rh, rc, eij, toij, eta, Pc, a.d.lambda[c], a.rel, a.dt, a.f.EII_pl[c]);
    a.f.txx[c] = o.v[0]; a.f.tyy[c] = o.v[1]; a.f.tzz[c] = o.v[2];
    a.f.tyz_c[c] = o.v[3]; a.f.txz_c[c] = o.v[4]; a.f.txy_c[c] = o.v[5];
    a.f.eplxx[c] = o.v[6]; a.f.eplyy[c] = o.v[7]; a.f.eplzz[c] = o.v[8];
    a.f.evol_pl[c] = o.v[L::EVOL];
    a.f.tII[c] = o.v[L::TII];
    a.f.eta_vep[c] = o.v[L::VEP];
    a.d.lambda[c] = o.v[L::LAM];
    a.d.dPpsi[c] = o.v[L::DP];
    a.d.P_num[c] = a.d.gamma_eff[c] * a.f.RP[c] + o.v[L::DP];      // θc = γ_eff RP + ΔPψ
    if (!LIN) {
        double T = 0.0;      // local_viscosity_args: T[I .+ 1] of the ghosted thermal.T
        if (mat_viscosity_reads_fields(&a.rh) && a.f.T) T = a.tg ? a.f.T[(i + 1) + (nx + 2) * ((j + 1) + (ny + 2) * (k + 1))] : a.f.T[c];
        a.f.eta[c] = dy_visc<6>(a.rh, a.nu, a.cut_lo, a.cut_hi, rc, o.v, T, Pc, eta);
    }
}

// one thread per node of ni .+ 1.  PART: bit T = edge family T, bit 3 = the centre of the same index
template <bool SOFT, bool LIN, int PART>
__global__ __launch_bounds__(256) void k_dy3_stress(const Dy3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    DY3_NODE(nx + 1, ny + 1)
    if (PART & 7) {
        const int ci[3] = {clampi(i - 1, 0, nx - 1), clampi(i, 0, nx - 1), clampi(i + 1, 0, nx - 1)};
        const int cj[3] = {clampi(j - 1, 0, ny - 1), clampi(j, 0, ny - 1), clampi(j + 1, 0, ny - 1)};
        const int ck[3] = {clampi(k - 1, 0, nz - 1), clampi(k, 0, nz - 1), clampi(k + 1, 0, nz - 1)};
        if ((PART & 1) && i < nx) dy3_edge_at<0, SOFT>(a, i, j, k, ci, cj, ck);
        if ((PART & 2) && j < ny) dy3_edge_at<1, SOFT>(a, i, j, k, ci, cj, ck);
        if ((PART & 4) && k < nz) dy3_edge_at<2, SOFT>(a, i, j, k, ci, cj, ck);
    }
    if ((PART & 8) && i < nx && j < ny && k < nz) dy3_centre_at<SOFT, LIN>(a, i, j, k);
}

// the momentum residuals: the 2D DYREL residual (MiniKernels.jl:37-72) one dimension up, on the index triples of src/stokes/VelocityKernels.jl:215-238;
// θ = ΔPψ (PH) or θc (DR)
struct Dy3Mom { const double *P, *th, *txx, *tyy, *tzz, *tyz, *txz, *txy, *fx, *fy, *fz; double _dx, _dy, _dz; int nx, ny, nz; };
__device__ __forceinline__ double dy3_Rx(const Dy3Mom &m, const int i, const int j, const int k)
{
    const int nx = m.nx, ny = m.ny, c = i + nx * (j + ny * k);
    return (-m.txx[c] + m.txx[c + 1]) * m._dx + (-EXY(m.txy, i + 1, j, k) + EXY(m.txy, i + 1, j + 1, k)) * m._dy + (-EXZ(m.txz, i + 1, j, k) + EXZ(m.txz, i + 1, j, k + 1)) * m._dz -
           (-m.P[c] + m.P[c + 1]) * m._dx - (-m.th[c] + m.th[c + 1]) * m._dx - (m.fx[c] + m.fx[c + 1]) * 0.5;
}
__device__ __forceinline__ double dy3_Ry(const Dy3Mom &m, const int i, const int j, const int k)
{
    const int nx = m.nx, ny = m.ny, c = i + nx * (j + ny * k);
    return (-m.tyy[c] + m.tyy[c + nx]) * m._dy + (-EXY(m.txy, i, j + 1, k) + EXY(m.txy, i + 1, j + 1, k)) * m._dx + (-EYZ(m.tyz, i, j + 1, k) + EYZ(m.tyz, i, j + 1, k + 1)) * m._dz -
           (-m.P[c] + m.P[c + nx]) * m._dy - (-m.th[c] + m.th[c + nx]) * m._dy - (m.fy[c] + m.fy[c + nx]) * 0.5;
}
__device__ __forceinline__ double dy3_Rz(const Dy3Mom &m, const int i, const int j, const int k)
{
    const int nx = m.nx, ny = m.ny, c = i + nx * (j + ny * k), cz = c + nx * ny;
    return (-m.tzz[c] + m.tzz[cz]) * m._dz + (-EXZ(m.txz, i, j, k + 1) + EXZ(m.txz, i + 1, j, k + 1)) * m._dx + (-EYZ(m.tyz, i, j, k + 1) + EYZ(m.tyz, i, j + 1, k + 1)) * m._dy -
           (-m.P[c] + m.P[cz]) * m._dz - (-m.th[c] + m.th[cz]) * m._dz - (m.fz[c] + m.fz[cz]) * 0.5;
}

// compute_PH_residual_V! 3D (velocity_kernels.jl:441-477, with the shear differences stated above): one thread per cell
__global__ __launch_bounds__(256) void k_dy3_ph_residual(const Dy3Mom m, double *__restrict__ Rx, double *__restrict__ Ry, double *__restrict__ Rz)
{
    const int nx = m.nx, ny = m.ny, nz = m.nz;
    DY3_NODE(nx, ny)
    if (i < nx - 1) Rx[i + (nx - 1) * (j + ny * k)] = dy3_Rx(m, i, j, k);
    if (j < ny - 1) Ry[i + nx * (j + (ny - 1) * k)] = dy3_Ry(m, i, j, k);
    if (k < nz - 1) Rz[i + nx * (j + ny * k)] = dy3_Rz(m, i, j, k);
}

// compute_DR_residual_update_V! 3D (velocity_kernels.jl:729-828): R / D, damped_update_V (:660-663), V; the ghosts are left to flow_bcs!
struct Dy3Upd { double *R[3], *V[3], *dVdtau[3]; const double *D[3], *al[3], *be[3], *dtau[3]; };
__device__ __forceinline__ void dy3_move(const Dy3Upd &u, const int c, const int n, const int q, const double raw)
{
    const double R = raw / u.D[c][n];
    u.R[c][n] = R;
    const double dnew = u.al[c][n] * u.dVdtau[c][n] + R;
    u.dVdtau[c][n] = dnew;
    u.V[c][q] = u.V[c][q] + dnew * u.be[c][n] * u.dtau[c][n];
}
__global__ __launch_bounds__(256) void k_dy3_update(const Dy3Mom m, const Dy3Upd u)
{
    const int nx = m.nx, ny = m.ny, nz = m.nz;
    DY3_NODE(nx, ny)
    if (i < nx - 1) dy3_move(u, 0, i + (nx - 1) * (j + ny * k), (i + 1) + (nx + 1) * ((j + 1) + (ny + 2) * (k + 1)), dy3_Rx(m, i, j, k));
    if (j < ny - 1) dy3_move(u, 1, i + nx * (j + (ny - 1) * k), (i + 1) + (nx + 2) * ((j + 1) + (ny + 1) * (k + 1)), dy3_Ry(m, i, j, k));
    if (k < nz - 1) dy3_move(u, 2, i + nx * (j + ny * k), (i + 1) + (nx + 2) * ((j + 1) + (ny + 2) * (k + 1)), dy3_Rz(m, i, j, k));
}

// The eigenvalue bound: Gershgorin_Stokes2D_SchurComplement! (Gershgorin.jl:21-155) one dimension up, no reference text.  One velocity node with its two normal
// neighbours (centres P / M: γ and the effective viscosity e) and its two pairs of shear neighbours (edges: effective viscosities a1 across spacing 1, a2 across 2):
//   D    = (a1P + a1M) / d1² + (a2P + a2M) / d2² + (γP + γM + 4/3 (eP + eM)) / dn²
//   Cnn  = |a1P| / d1² + |a1M| / d1² + |a2P| / d2² + |a2M| / d2² + |γP + 4/3 eP| / dn² + |γM + 4/3 eM| / dn² + |D|
//   Cn1  = (|γP - 2/3 eP + a1P| + |γP - 2/3 eP + a1M| + |γM - 2/3 eM + a1P| + |γM - 2/3 eM + a1M|) / (dn d1), Cn2 alike;   λmax = (Cnn + Cn1 + Cn2) / D
// in the 2D kernel's order of operations.  Vx: shear pairs xy (N / S, dy) and xz (T / B, dz); Vy and Vz by cyclic permutation: yz (dz) and xy (dx); xz (dx) and yz (dy).
struct Dy3G { double D, lmax; };
__device__ __forceinline__ Dy3G dy3_gersh(const double gP, const double gM, const double eP, const double eM, const double a1P, const double a1M, const double a2P,
                                          const double a2M, const double _dn, const double _d1, const double _d2)
{
    const double c43 = 4.0 / 3.0, c23 = 2.0 / 3.0;
    const double _dn2 = _dn * _dn, _d12 = _d1 * _d1, _d22 = _d2 * _d2, _dnd1 = _dn * _d1, _dnd2 = _dn * _d2;
    const double a1P_d = a1P * _d1, a1M_d = a1M * _d1, a2P_d = a2P * _d2, a2M_d = a2M * _d2, eP_d = eP * _dn, eM_d = eM * _dn, gP_d = gP * _dn, gM_d = gM * _dn;
    const double D = (a1P_d + a1M_d) * _d1 + (a2P_d + a2M_d) * _d2 + (gP_d + gM_d + c43 * (eP_d + eM_d)) * _dn;
    const double Cnn = fabs(a1P * _d12) + fabs(a1M * _d12) + fabs(a2P * _d22) + fabs(a2M * _d22) + fabs((gP + c43 * eP) * _dn2) + fabs((gM + c43 * eM) * _dn2) + fabs(D);
    const double Cn1 = fabs((gP - c23 * eP + a1P) * _dnd1) + fabs((gP - c23 * eP + a1M) * _dnd1) + fabs((gM + a1P - c23 * eM) * _dnd1) + fabs((gM + a1M - c23 * eM) * _dnd1);
    const double Cn2 = fabs((gP - c23 * eP + a2P) * _dnd2) + fabs((gP - c23 * eP + a2M) * _dnd2) + fabs((gM + a2P - c23 * eM) * _dnd2) + fabs((gM + a2M - c23 * eM) * _dnd2);
    return Dy3G{D, (1 / D) * (Cnn + Cn1 + Cn2)};
}
// the effective viscosity 1 / (1 / η + 1 / (G dt)) of the edge (i, j, k) of family T: η = harm_clamped_*(η), the stress kernel's; G from the edge's own ratios
template <int T>
__device__ __forceinline__ double dy3_edge_ve(const Dy3Args &a, const int i, const int j, const int k)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz, np = a.rh.nphase;
    const int ci[2] = {clampi(i - 1, 0, nx - 1), clampi(i, 0, nx - 1)}, cj[2] = {clampi(j - 1, 0, ny - 1), clampi(j, 0, ny - 1)}, ck[2] = {clampi(k - 1, 0, nz - 1), clampi(k, 0, nz - 1)};
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double inv = 1 / a.f.eta[ci[cen3(T, q, 0)] + nx * (cj[cen3(T, q, 1)] + ny * ck[cen3(T, q, 2)])];
        s = q == 0 ? inv : s + inv;
    }
    const double e = 4 / s;
    const int n1 = nx + (T != 0), n2 = ny + (T != 1);
    const double *ph = T == 0 ? a.f.phase_yz : (T == 1 ? a.f.phase_xz : a.f.phase_xy);
    const double G = ratio_avg(a.rh.G, ph + np * (i + n1 * (j + n2 * k)), np);
    return 1 / (1 / e + 1 / (G * a.dt));
}
__global__ __launch_bounds__(256) void k_dy3_gershgorin(const Dy3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz, np = a.rh.nphase;
    DY3_NODE(nx, ny)
    const int c = i + nx * (j + ny * k);
    const double *__restrict__ eta = a.f.eta, *__restrict__ gam = a.d.gamma_eff;
#define VEC(c_) (1 / (1 / eta[c_] + 1 / (ratio_avg(a.rh.G, a.f.phase_c + np * (c_), np) * a.dt)))
    const double e_c = VEC(c), g_c = gam[c];
    if (i < nx - 1) {
        const Dy3G g = dy3_gersh(gam[c + 1], g_c, VEC(c + 1), e_c, dy3_edge_ve<2>(a, i + 1, j + 1, k), dy3_edge_ve<2>(a, i + 1, j, k), dy3_edge_ve<1>(a, i + 1, j, k + 1),
                                 dy3_edge_ve<1>(a, i + 1, j, k), a._dx, a._dy, a._dz);
        const int n = i + (nx - 1) * (j + ny * k);
        a.d.Dx[n] = g.D; a.d.lmaxVx[n] = g.lmax;
    }
    if (j < ny - 1) {
        const Dy3G g = dy3_gersh(gam[c + nx], g_c, VEC(c + nx), e_c, dy3_edge_ve<0>(a, i, j + 1, k + 1), dy3_edge_ve<0>(a, i, j + 1, k), dy3_edge_ve<2>(a, i + 1, j + 1, k),
                                 dy3_edge_ve<2>(a, i, j + 1, k), a._dy, a._dz, a._dx);
        const int n = i + nx * (j + (ny - 1) * k);
        a.d.Dy[n] = g.D; a.d.lmaxVy[n] = g.lmax;
    }
    if (k < nz - 1) {
        const Dy3G g = dy3_gersh(gam[c + nx * ny], g_c, VEC(c + nx * ny), e_c, dy3_edge_ve<1>(a, i + 1, j, k + 1), dy3_edge_ve<1>(a, i, j, k + 1), dy3_edge_ve<0>(a, i, j + 1, k + 1),
                                 dy3_edge_ve<0>(a, i, j, k + 1), a._dz, a._dx, a._dy);
        a.d.Dz[c] = g.D; a.d.lmaxVz[c] = g.lmax;
    }
#undef VEC
}

// _update_dτV_α_β! (Gershgorin.jl:229-247, 290-310; DTAU) / _update_α_β! (:182-198): the reference's @muladd is the two fma here
struct Dy3Damp { double *dtau[3], *beta[3], *alpha[3]; const double *cV[3], *lmax[3]; int n[3]; };
template <bool DTAU>
__global__ __launch_bounds__(256) void k_dy3_dtau(const Dy3Damp d, const double CFL)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (t >= d.n[c]) continue;
        double x = d.dtau[c][t];
        if (DTAU) { x = 2 / sqrt(d.lmax[c][t]) * CFL; d.dtau[c][t] = x; }
        const double cv = d.cV[c][t], den = fma(cv, x, 2.0);
        d.beta[c][t] = 2 * x / den;
        d.alpha[c][t] = fma(-cv, x, 2.0) / den;
    }
}

// compute_bulk_viscosity_and_penalty! (constructors.jl:237-254); eta_mean = mean(η[.!isinf.(η)]) is sums[0] / sums[1] of k_dy3_eta_sum
__global__ __launch_bounds__(256) void k_dy3_bulk(const Dy3Args a, const double *__restrict__ sums, const double gamma_fact)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.nx * a.ny * a.nz) return;
    const double eta_mean = sums[0] / sums[1];
    const double Kbdt = ratio_avg(a.rh.Kb, a.f.phase_c + a.rh.nphase * t, a.rh.nphase) * a.dt;
    a.d.etab[t] = Kbdt;
    const double e = a.f.eta[t];
    const double g_num = gamma_fact * (isinf(e) ? eta_mean : e);
    const double g_phy = isinf(Kbdt) ? g_num : Kbdt;
    a.d.gamma_eff[t] = g_phy * g_num / (g_phy + g_num);
}

// fixed-order two-stage sums, no atomics: wave shuffle -> the four waves of a block -> one partial row of DY3_NS per block -> k_dy3_sum_final in one block
constexpr int DY3_NS = 12;
__device__ __forceinline__ void dy3_block_store(const double s[DY3_NS], const int ns, double *__restrict__ partials)
{
    __shared__ double sm[DY3_NS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < ns; c++) {
        const double w = wave_sum(s[c]);
        if (lane == 0) sm[c][wave] = w;
    }
    __syncthreads();
    if ((int)threadIdx.x < DY3_NS) {
        const int c = threadIdx.x;
        partials[blockIdx.x * DY3_NS + c] = c < ns ? (sm[c][0] + sm[c][1]) + (sm[c][2] + sm[c][3]) : 0.0;
    }
}
__global__ __launch_bounds__(256) void k_dy3_sum_final(const double *__restrict__ partials, const int nblocks, double *__restrict__ out)
{
    __shared__ double sm[DY3_NS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < DY3_NS; c++) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += partials[b * DY3_NS + c];
        s = wave_sum(s);
        if (lane == 0) sm[c][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < DY3_NS) {
        const int c = threadIdx.x;
        out[c] = (sm[c][0] + sm[c][1]) + (sm[c][2] + sm[c][3]);
    }
}
// Σ η and the count over the finite entries
__global__ __launch_bounds__(256) void k_dy3_eta_sum(const double *__restrict__ eta, const int n, double *__restrict__ partials)
{
    double s[DY3_NS] = {};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const double e = eta[t];
        if (!isinf(e)) { s[0] += e; s[1] += 1.0; }
    }
    dy3_block_store(s, 2, partials);
}
// the Powell-Hestenes norms (solver.jl:151-152): Σ Rx², Σ Ry², Σ Rz², Σ RP² over the whole arrays
__global__ __launch_bounds__(256) void k_dy3_ph_sums(const double *__restrict__ Rx, const double *__restrict__ Ry, const double *__restrict__ Rz, const double *__restrict__ RP,
                                                     const int nxn, const int nyn, const int nzn, const int n, double *__restrict__ partials)
{
    double s[DY3_NS] = {};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        if (t < nxn) { const double v = Rx[t]; s[0] += v * v; }
        if (t < nyn) { const double v = Ry[t]; s[1] += v * v; }
        if (t < nzn) { const double v = Rz[t]; s[2] += v * v; }
        const double v = RP[t];
        s[3] += v * v;
    }
    dy3_block_store(s, 4, partials);
}
// the residual check of the inner loop (solver.jl:231,251, :359-365): compute_dV!, then per component Σ (D R)², Σ dV (R - R0), Σ dV²
struct Dy3Chk { double *dV[3]; const double *R[3], *R0[3], *D[3], *dVdtau[3], *be[3], *dtau[3]; int n[3]; };
__global__ __launch_bounds__(256) void k_dy3_check_sums(const Dy3Chk d, const int nmax, double *__restrict__ partials)
{
    double s[DY3_NS] = {};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nmax; t += gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (t >= d.n[c]) continue;
            const double R = d.R[c][t], DR = d.D[c][t] * R, dV = d.dVdtau[c][t] * d.be[c][t] * d.dtau[c][t];
            d.dV[c][t] = dV;
            s[c] += DR * DR; s[3 + c] += dV * (R - d.R0[c][t]); s[6 + c] += dV * dV;
        }
    }
    dy3_block_store(s, 9, partials);
}
// update_cV! (velocity_kernels.jl:642-654)
__global__ __launch_bounds__(256) void k_dy3_fill3(double *__restrict__ a0, const int n0, double *__restrict__ a1, const int n1, double *__restrict__ a2, const int n2,
                                                   const double v)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n0) a0[t] = v;
    if (t < n1) a1[t] = v;
    if (t < n2) a2[t] = v;
}
// @. P += γ_eff * RP (solver.jl:264)
__global__ __launch_bounds__(256) void k_dy3_add_P(double *__restrict__ P, const double *__restrict__ gam, const double *__restrict__ RP, const int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) P[t] = P[t] + gam[t] * RP[t];
}
// the epilogue (solver.jl:269-286): P += ΔPψ, compute_∇V!, compute_vorticity! 3D, shear2center! of ε, ε_pl, Δε, accumulate_tensor!, accumulate_vol!; one thread per
// node of ni .+ 1.  P, EII_pl and EVol_pl are updated in place at the thread's own cell; everything a neighbour reads (V, the edge arrays) is not written
__global__ __launch_bounds__(256) void k_dy3_epilogue(const Dy3Args a)
{
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    DY3_NODE(nx + 1, ny + 1)
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy, *__restrict__ Vz = a.f.Vz;
    // compute_vorticity! 3D (stress_rotation_particles.jl:31-50)
    if (a.f.omega_yz && i < nx) EYZ(a.f.omega_yz, i, j, k) = 0.5 * ((-VZ(i, j, k) + VZ(i, j + 1, k)) * a._dy - (-VY(i, j, k) + VY(i, j, k + 1)) * a._dz);
    if (a.f.omega_xz && j < ny) EXZ(a.f.omega_xz, i, j, k) = 0.5 * ((-VX(i, j, k) + VX(i, j, k + 1)) * a._dz - (-VZ(i, j, k) + VZ(i + 1, j, k)) * a._dx);
    if (a.f.omega_xy && k < nz) EXY(a.f.omega_xy, i, j, k) = 0.5 * ((-VY(i, j, k) + VY(i + 1, j, k)) * a._dx - (-VX(i, j, k) + VX(i, j + 1, k)) * a._dy);
    if (i < nx && j < ny && k < nz) {
        const int c = i + nx * (j + ny * k);
        a.f.P[c] = a.f.P[c] + a.d.dPpsi[c];
        a.f.divV[c] = (-VX(i, j + 1, k + 1) + VX(i + 1, j + 1, k + 1)) * a._dx + (-VY(i + 1, j, k + 1) + VY(i + 1, j + 1, k + 1)) * a._dy +
                      (-VZ(i + 1, j + 1, k) + VZ(i + 1, j + 1, k + 1)) * a._dz;
        // shear2center! (Interpolations.jl:314-323) of ε, ε_pl, Δε
#define S2C(dst, yz, xz, xy, M, arr) if (dst) (dst)[c] = 0.25 * (M(arr, i, j, k) + M(arr, i + (xz | xy), j + yz, k) + M(arr, i, j + xy, k + (yz | xz)) + M(arr, i + (xz | xy), j + (yz | xy), k + (yz | xz)))
        S2C(a.f.eyz_c, 1, 0, 0, EYZ, a.f.eyz); S2C(a.f.exz_c, 0, 1, 0, EXZ, a.f.exz); S2C(a.f.exy_c, 0, 0, 1, EXY, a.f.exy);
        S2C(a.f.eplyz_c, 1, 0, 0, EYZ, a.f.eplyz); S2C(a.f.eplxz_c, 0, 1, 0, EXZ, a.f.eplxz); S2C(a.f.eplxy_c, 0, 0, 1, EXY, a.f.eplxy);
        if (a.f.deyz && a.f.dexz && a.f.dexy) { S2C(a.f.deyz_c, 1, 0, 0, EYZ, a.f.deyz); S2C(a.f.dexz_c, 0, 1, 0, EXZ, a.f.dexz); S2C(a.f.dexy_c, 0, 0, 1, EXY, a.f.dexy); }
#undef S2C
        // accumulate_tensor! (second_invariant_staggered: the mean of the squared edge values, StressKernels.jl:394-408) and accumulate_vol! (:410-431)
        const double *yz = a.f.eplyz, *xz = a.f.eplxz, *xy = a.f.eplxy;
        const double a0 = EYZ(yz, i, j, k), a1 = EYZ(yz, i, j + 1, k), a2 = EYZ(yz, i, j, k + 1), a3 = EYZ(yz, i, j + 1, k + 1);
        const double b0 = EXZ(xz, i, j, k), b1 = EXZ(xz, i + 1, j, k), b2 = EXZ(xz, i, j, k + 1), b3 = EXZ(xz, i + 1, j, k + 1);
        const double c0 = EXY(xy, i, j, k), c1 = EXY(xy, i + 1, j, k), c2 = EXY(xy, i, j + 1, k), c3 = EXY(xy, i + 1, j + 1, k);
        const double syz = 0.25 * (a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3), sxz = 0.25 * (b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3), sxy = 0.25 * (c0 * c0 + c1 * c1 + c2 * c2 + c3 * c3);
        const double xx = a.f.eplxx[c], yy = a.f.eplyy[c], zz = a.f.eplzz[c];
        a.f.EII_pl[c] += sqrt(0.5 * (xx * xx + yy * yy + zz * zz) + syz + sxz + sxy) * a.dt;
        a.f.EVol_pl[c] += a.dt * a.f.evol_pl[c];
    }
}
#undef VX
#undef VY
#undef VZ

// what every 3D DYREL entry point refuses (status JRX_ERR_ARG, each named), before anything is launched
jrx_status dy3_check(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh, const jrx_vep3d_params *p)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !d || !p) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    JRX_TRY(jrx_check_device(h));
    if (jrx_comm_active(h)) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: a communicator of more than one rank is not built (single block only)");
    for (const double x : {p->_dx, p->_dy, p->_dz})
        if (!(x > 0.0) || std::isinf(x))
            return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: a non-uniform Geometry is not built (the inverse spacings must be positive finite scalars)");
    if (phi) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: the variational form with a RockRatio is not built");
    if (d->dT) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: the thermal form of the pressure residual (args.ΔT) is not built");
    if (d->melt_fraction) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: the melt-fraction form of the pressure residual (args.melt_fraction) is not built");
    if (p->periodic) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: periodic velocity boundary conditions are not built");
    if (p->displacement_bcs < 0)      // jrx_vep3d_params has no free_surface member: a binding hands flow_bcs.free_surface over as displacement_bcs = -1
        return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: a free_surface boundary condition (free-surface stabilisation) is not built");
    if (p->nx < 3 || p->ny < 3 || p->nz < 3) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: needs at least 3 cells per dimension");
    if (rh) {
        if (rh->nphase < 1 || rh->nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "nphase must be in 1..%d", JRX_MAXPHASE);
        for (int q = 0; q < rh->nphase; q++)
            if (rh->is_pl[q] != 0 && rh->is_pl[q] != 1)
                return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: is_pl = %d of phase %d is not built (0 or 1: none, DruckerPrager_regularised)", (int)rh->is_pl[q], q);
    }
    if ((double)(p->nx + 2) * (double)(p->ny + 2) * (double)(p->nz + 2) * (double)(rh ? rh->nphase : 1) >= 2147483648.0)
        return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: an array of 2^31 or more entries exceeds the 32-bit offsets of its kernels");
    return JRX_OK;
}

Dy3Args dy3_make(const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p)
{
    Dy3Args a;
    memset(&a, 0, sizeof(a));
    a.f = *f; a.d = *d;
    if (rh) a.rh = *rh;
    a._dx = p->_dx; a._dy = p->_dy; a._dz = p->_dz; a.dt = p->dt;
    a.nx = (int)p->nx; a.ny = (int)p->ny; a.nz = (int)p->nz;
    a.fs = p->free_slip; a.ns = p->no_slip;
    a.tg = p->T_ghosted != 0;
    a.rel = 1.0; a.nu = 1.0e-2; a.cut_lo = -INFINITY; a.cut_hi = INFINITY;
    return a;
}
Dy3Mom dy3_mom(const Dy3Args &a, const double *th)
{
    return Dy3Mom{a.f.P, th, a.f.txx, a.f.tyy, a.f.tzz, a.f.tyz, a.f.txz, a.f.txy, a.f.fx, a.f.fy, a.f.fz, a._dx, a._dy, a._dz, a.nx, a.ny, a.nz};
}
Dy3Upd dy3_upd(const Dy3Args &a)
{
    const jrx_dyrel3d_fields &d = a.d;
    return Dy3Upd{{a.f.Rx, a.f.Ry, a.f.Rz}, {a.f.Vx, a.f.Vy, a.f.Vz}, {d.dVxdtau, d.dVydtau, d.dVzdtau}, {d.Dx, d.Dy, d.Dz}, {d.alphaVx, d.alphaVy, d.alphaVz},
                  {d.betaVx, d.betaVy, d.betaVz}, {d.dtauVx, d.dtauVy, d.dtauVz}};
}
struct Dy3N { int c, x, y, z, max; };
Dy3N dy3_counts(const Dy3Args &a)
{
    Dy3N n{a.nx * a.ny * a.nz, (a.nx - 1) * a.ny * a.nz, a.nx * (a.ny - 1) * a.nz, a.nx * a.ny * (a.nz - 1), 0};
    n.max = n.x > n.y ? n.x : n.y;
    n.max = n.z > n.max ? n.z : n.max;
    return n;
}
bool dy3_has(std::initializer_list<const void *> req)
{
    for (const void *q : req)
        if (!q) return false;
    return true;
}
#define DY3_REQ(h, what, ...) \
    if (!dy3_has({__VA_ARGS__})) return jrx_fail(h, JRX_ERR_ARG, "%s: a required field pointer is NULL", what)
#define DY3_LAUNCH(h) \
    do { (h)->stat_dyrel_launches++; JRX_LAUNCH_CHECK(h); } while (0)

inline dim3 dy3_gv(const Dy3Args &a) { return DY3_GRID(a.nx + 1, a.ny + 1, a.nz + 1); }
inline dim3 dy3_gc(const Dy3Args &a) { return DY3_GRID(a.nx, a.ny, a.nz); }
inline unsigned dy3_g1(int n) { return (unsigned)((n + 255) / 256); }
inline int dy3_nblk(const Dy3Args &a) { const unsigned g = (dy3_g1(a.nx * a.ny * a.nz) + 7) / 8; return (int)(g < 1 ? 1 : (g > 512 ? 512 : g)); }      // partial rows of 12: 512 rows fit kMaxRedBlocks rows of 4
static_assert(512 * DY3_NS <= kMaxRedBlocks * 4, "the reduction scratch holds the partial rows");

jrx_status dy3_strain_rp(jrx_handle *h, hipStream_t s, const Dy3Args &a, bool strain)
{
    const jrx_vep3d_fields &f = a.f;
    if (strain) hipLaunchKernelGGL(k_dy3_strain_rp<true>, dy3_gv(a), dim3(256), 0, s, f.exx, f.eyy, f.ezz, f.eyz, f.exz, f.exy, (const double *)f.Vx, (const double *)f.Vy,
                                   (const double *)f.Vz, f.RP, (const double *)f.P, (const double *)f.P0, (const double *)f.Q, (const double *)a.d.etab, a._dx, a._dy, a._dz,
                                   a.dt, a.nx, a.ny, a.nz);
    else hipLaunchKernelGGL(k_dy3_strain_rp<false>, dy3_gv(a), dim3(256), 0, s, f.exx, f.eyy, f.ezz, f.eyz, f.exz, f.exy, (const double *)f.Vx, (const double *)f.Vy,
                            (const double *)f.Vz, f.RP, (const double *)f.P, (const double *)f.P0, (const double *)f.Q, (const double *)a.d.etab, a._dx, a._dy, a._dz, a.dt,
                            a.nx, a.ny, a.nz);
    DY3_LAUNCH(h);
    return JRX_OK;
}
template <bool SOFT, bool LIN>
jrx_status dy3_stress_t(jrx_handle *h, hipStream_t s, const Dy3Args &a)
{
    hipLaunchKernelGGL((k_dy3_stress<SOFT, LIN, 7>), dy3_gv(a), dim3(256), 0, s, a);
    DY3_LAUNCH(h);
    hipLaunchKernelGGL((k_dy3_stress<SOFT, LIN, 8>), dy3_gc(a), dim3(256), 0, s, a);
    DY3_LAUNCH(h);
    return JRX_OK;
}
jrx_status dy3_stress(jrx_handle *h, hipStream_t s, const Dy3Args &a, bool lin)
{
    if (mat_has_softening(&a.rh)) return lin ? dy3_stress_t<true, true>(h, s, a) : dy3_stress_t<true, false>(h, s, a);
    return lin ? dy3_stress_t<false, true>(h, s, a) : dy3_stress_t<false, false>(h, s, a);
}
jrx_status dy3_gershgorin(jrx_handle *h, hipStream_t s, const Dy3Args &a)
{
    hipLaunchKernelGGL(k_dy3_gershgorin, dy3_gc(a), dim3(256), 0, s, a);
    DY3_LAUNCH(h);
    return JRX_OK;
}
jrx_status dy3_dtau(jrx_handle *h, hipStream_t s, const Dy3Args &a, double CFL, bool from_lmax)
{
    const jrx_dyrel3d_fields &d = a.d;
    const Dy3N n = dy3_counts(a);
    const Dy3Damp q{{d.dtauVx, d.dtauVy, d.dtauVz}, {d.betaVx, d.betaVy, d.betaVz}, {d.alphaVx, d.alphaVy, d.alphaVz}, {d.cVx, d.cVy, d.cVz}, {d.lmaxVx, d.lmaxVy, d.lmaxVz},
                    {n.x, n.y, n.z}};
    if (from_lmax) hipLaunchKernelGGL(k_dy3_dtau<true>, dim3(dy3_g1(n.max)), dim3(256), 0, s, q, CFL);
    else hipLaunchKernelGGL(k_dy3_dtau<false>, dim3(dy3_g1(n.max)), dim3(256), 0, s, q, CFL);
    DY3_LAUNCH(h);
    return JRX_OK;
}
jrx_status dy3_bulk(jrx_handle *h, hipStream_t s, const Dy3Args &a, double gamma_fact)
{
    const int nb = dy3_nblk(a), n = a.nx * a.ny * a.nz;
    hipLaunchKernelGGL(k_dy3_eta_sum, dim3(nb), dim3(256), 0, s, (const double *)a.f.eta, n, h->d_partials);
    DY3_LAUNCH(h);
    hipLaunchKernelGGL(k_dy3_sum_final, dim3(1), dim3(256), 0, s, (const double *)h->d_partials, nb, h->d_sums);
    DY3_LAUNCH(h);
    hipLaunchKernelGGL(k_dy3_bulk, dim3(dy3_g1(n)), dim3(256), 0, s, a, (const double *)h->d_sums, gamma_fact);
    DY3_LAUNCH(h);
    return JRX_OK;
}
// DYREL! (constructors.jl:178-190)
jrx_status dy3_init(jrx_handle *h, hipStream_t s, const Dy3Args &a, double CFL, double gamma_fact)
{
    JRX_TRY(dy3_bulk(h, s, a, gamma_fact));
    JRX_TRY(dy3_gershgorin(h, s, a));
    return dy3_dtau(h, s, a, CFL, true);
}
// the sums of one reduction kernel, read on the host: the one synchronisation of a check
jrx_status dy3_read_sums(jrx_handle *h, hipStream_t s, int nb, int count)
{
    hipLaunchKernelGGL(k_dy3_sum_final, dim3(1), dim3(256), 0, s, (const double *)h->d_partials, nb, h->d_sums);
    DY3_LAUNCH(h);
    JRX_HIP(h, hipMemcpyAsync(h->h_sums, h->d_sums, count * sizeof(double), hipMemcpyDeviceToHost, s));
    JRX_HIP(h, hipStreamSynchronize(s));
    return JRX_OK;
}

#define DY3_FIELDS_STRESS(f, d)                                                                                                                                     \
    (f)->P, (f)->exx, (f)->eyy, (f)->ezz, (f)->eyz, (f)->exz, (f)->exy, (f)->eplxx, (f)->eplyy, (f)->eplzz, (f)->eplyz, (f)->eplxz, (f)->eplxy, (f)->txx, (f)->tyy,    \
        (f)->tzz, (f)->tyz, (f)->txz, (f)->txy, (f)->tyz_c, (f)->txz_c, (f)->txy_c, (f)->tII, (f)->toxx, (f)->toyy, (f)->tozz, (f)->toyz, (f)->toxz, (f)->toxy,       \
        (f)->toyz_c, (f)->toxz_c, (f)->toxy_c, (f)->eta, (f)->eta_vep, (f)->EII_pl, (f)->evol_pl, (f)->RP, (f)->phase_c, (f)->phase_yz, (f)->phase_xz, (f)->phase_xy, \
        (d)->lambda, (d)->lambda_yz, (d)->lambda_xz, (d)->lambda_xy, (d)->dPpsi, (d)->P_num, (d)->gamma_eff
#define DY3_FIELDS_MOM(f) (f)->P, (f)->txx, (f)->tyy, (f)->tzz, (f)->tyz, (f)->txz, (f)->txy, (f)->fx, (f)->fy, (f)->fz, (f)->Rx, (f)->Ry, (f)->Rz
#define DY3_FIELDS_DAMP(d)                                                                                                                                          \
    (d)->Dx, (d)->Dy, (d)->Dz, (d)->lmaxVx, (d)->lmaxVy, (d)->lmaxVz, (d)->dVxdtau, (d)->dVydtau, (d)->dVzdtau, (d)->dtauVx, (d)->dtauVy, (d)->dtauVz, (d)->dVx,       \
        (d)->dVy, (d)->dVz, (d)->betaVx, (d)->betaVy, (d)->betaVz, (d)->cVx, (d)->cVy, (d)->cVz, (d)->alphaVx, (d)->alphaVy, (d)->alphaVz, (d)->Rx0, (d)->Ry0, (d)->Rz0

}   // namespace

extern "C" {

jrx_status jrx_dyrel3d_strain_rate_RP(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p, int32_t do_strain_rate)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, nullptr, p));
    DY3_REQ(h, "compute_∇V_strain_rate_RP! 3D", f->exx, f->eyy, f->ezz, f->eyz, f->exz, f->exy, f->Vx, f->Vy, f->Vz, f->RP, f->P, f->P0, f->Q, d->etab);
    const Dy3Args a = dy3_make(f, d, nullptr, p);
    JRX_TRY(dy3_strain_rp(h, h->stream, a, do_strain_rate != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_stress_viscosity(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p,
                                        const jrx_dyrel2d_params *dp, double lambda_relaxation)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, rh, p));
    if (!rh || !dp) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY3_REQ(h, "compute_stress_viscosity_DRYEL! 3D", DY3_FIELDS_STRESS(f, d));
    Dy3Args a = dy3_make(f, d, rh, p);
    a.rel = lambda_relaxation; a.nu = dp->viscosity_relaxation; a.cut_lo = dp->cutoff_lo; a.cut_hi = dp->cutoff_hi;
    JRX_TRY(dy3_stress(h, h->stream, a, dp->linear_viscosity != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_PH_residual(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, nullptr, p));
    DY3_REQ(h, "compute_PH_residual_V! 3D", DY3_FIELDS_MOM(f), d->dPpsi);
    const Dy3Args a = dy3_make(f, d, nullptr, p);
    hipLaunchKernelGGL(k_dy3_ph_residual, dy3_gc(a), dim3(256), 0, h->stream, dy3_mom(a, d->dPpsi), f->Rx, f->Ry, f->Rz);
    DY3_LAUNCH(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_DR_residual_update_V(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, nullptr, p));
    DY3_REQ(h, "compute_DR_residual_update_V! 3D", DY3_FIELDS_MOM(f), f->Vx, f->Vy, f->Vz, d->P_num, d->Dx, d->Dy, d->Dz, d->dVxdtau, d->dVydtau, d->dVzdtau, d->alphaVx,
            d->alphaVy, d->alphaVz, d->betaVx, d->betaVy, d->betaVz, d->dtauVx, d->dtauVy, d->dtauVz);
    const Dy3Args a = dy3_make(f, d, nullptr, p);
    hipLaunchKernelGGL(k_dy3_update, dy3_gc(a), dim3(256), 0, h->stream, dy3_mom(a, d->P_num), dy3_upd(a));
    DY3_LAUNCH(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_gershgorin(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, rh, p));
    if (!rh) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY3_REQ(h, "the 3D Gershgorin estimate", f->eta, f->phase_c, f->phase_yz, f->phase_xz, f->phase_xy, d->gamma_eff, d->Dx, d->Dy, d->Dz, d->lmaxVx, d->lmaxVy, d->lmaxVz);
    const Dy3Args a = dy3_make(f, d, rh, p);
    JRX_TRY(dy3_gershgorin(h, h->stream, a));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_update_dtauV_alpha_beta(jrx_handle *h, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p, double CFL, int32_t from_lambda_max)
{
    jrx_vep3d_fields none;
    memset(&none, 0, sizeof(none));
    JRX_TRY(dy3_check(h, &none, d, nullptr, nullptr, p));
    DY3_REQ(h, "update_dτV_α_β! 3D", d->dtauVx, d->dtauVy, d->dtauVz, d->betaVx, d->betaVy, d->betaVz, d->alphaVx, d->alphaVy, d->alphaVz, d->cVx, d->cVy, d->cVz, d->lmaxVx,
            d->lmaxVy, d->lmaxVz);
    const Dy3Args a = dy3_make(&none, d, nullptr, p);
    JRX_TRY(dy3_dtau(h, h->stream, a, CFL, from_lambda_max != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_bulk_viscosity_and_penalty(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh,
                                                  const jrx_vep3d_params *p, double gamma_fact)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, rh, p));
    if (!rh) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY3_REQ(h, "compute_bulk_viscosity_and_penalty! 3D", f->eta, f->phase_c, d->etab, d->gamma_eff);
    const Dy3Args a = dy3_make(f, d, rh, p);
    JRX_TRY(dy3_bulk(h, h->stream, a, gamma_fact));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_init(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                            const jrx_vep3d_params *p, const jrx_dyrel2d_params *dp)
{
    JRX_TRY(dy3_check(h, f, d, phi, rh, p));
    if (!rh || !dp) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY3_REQ(h, "DYREL! 3D", f->eta, f->phase_c, f->phase_yz, f->phase_xz, f->phase_xy, d->gamma_eff, d->etab, DY3_FIELDS_DAMP(d));
    const Dy3Args a = dy3_make(f, d, rh, p);
    JRX_TRY(dy3_init(h, h->stream, a, dp->CFL, dp->gamma_fact));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_solve(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                             const jrx_vep3d_params *p, const jrx_dyrel2d_params *dp, jrx_dyrel2d_result *res)
{
    JRX_TRY(dy3_check(h, f, d, phi, rh, p));
    if (!rh || !dp || !res) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    if (dp->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    DY3_REQ(h, "solve_DYREL! 3D", DY3_FIELDS_STRESS(f, d), DY3_FIELDS_MOM(f), DY3_FIELDS_DAMP(d), f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Vz, f->eplyz_c, f->eplxz_c,
            f->eplxy_c, f->EVol_pl, d->etab);
    if (mat_viscosity_reads_invariant(rh) && !(f->eyz_c && f->exz_c && f->exy_c)) return jrx_fail(h, JRX_ERR_ARG, "a power-law creep needs the centre shear strain rates for compute_viscosity!");
    hipStream_t s = h->stream;
    Dy3Args a = dy3_make(f, d, rh, p);
    a.nu = dp->viscosity_relaxation; a.cut_lo = dp->cutoff_lo; a.cut_hi = dp->cutoff_hi;
    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const Dy3N cnt = dy3_counts(a);
    const size_t n = (size_t)cnt.c;
    const EdgeN ne = edge_counts(nx, ny, nz);
    const bool lin = dp->linear_viscosity != 0;
    const int nb = dy3_nblk(a);
    const double EPS = 2.220446049250313e-16;
    // velocity_dofs(Val(3)), pressure_dof (solver.jl:349-357)
    const double dofs[3] = {(double)((p->nxg - 2) * (p->nyg - 1) * (p->nzg - 1)), (double)((p->nxg - 1) * (p->nyg - 2) * (p->nzg - 1)),
                            (double)((p->nxg - 1) * (p->nyg - 1) * (p->nzg - 2))};
    const double pdof = (double)(p->nxg * p->nyg * p->nzg);

    // solver.jl:86-95: P0 <- P, @tensor_center(ε_pl) = 0, λ = λv = 0
    JRX_HIP(h, hipMemcpyAsync(f->P0, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (double *q : {f->eplxx, f->eplyy, f->eplzz, f->eplyz_c, f->eplxz_c, f->eplxy_c, d->lambda}) JRX_HIP(h, hipMemsetAsync(q, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_yz, 0, (size_t)ne.yz * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_xz, 0, (size_t)ne.xz * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_xy, 0, (size_t)ne.xy * sizeof(double), s));
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    {   // :117-119: compute_viscosity! (relaxation 1, the strain-rate invariant), compute_ρg!(ρg[end], ...), DYREL!
        jrx_vep3d_params pv = *p;
        pv.cutoff_lo = dp->cutoff_lo; pv.cutoff_hi = dp->cutoff_hi;
        JRX_TRY(jrx_vep3d_compute_viscosity(h, f, rh, &pv, 1.0));
    }
    const int64_t nn[3] = {nx, ny, nz}, tdim[3] = {a.tg ? nx + 2 : nx, a.tg ? ny + 2 : ny, a.tg ? nz + 2 : nz};
    if (rh->has_density) JRX_TRY(jrx_compute_rhog(h, f->fz, rh, f->phase_c, f->T, f->P, nn, tdim, 3));
    JRX_TRY(dy3_init(h, s, a, dp->CFL, dp->gamma_fact));
    const bool rho_loop = rh->has_density && !mat_density_is_constant(rh);

    double err = 2 * dp->eps, err_min = INFINITY, errV0[3] = {1.0, 1.0, 1.0}, errPt0 = 1.0, errV00 = 1.0, errPt = 1.0, rel_drop = dp->rel_drop;
    int64_t iter = 0, cont = 0, itPH_done = 0;
    bool bcs_applied = false;
    jrx_status bad = JRX_OK;
    const Dy3Chk chk{{d->dVx, d->dVy, d->dVz}, {f->Rx, f->Ry, f->Rz}, {d->Rx0, d->Ry0, d->Rz0}, {d->Dx, d->Dy, d->Dz}, {d->dVxdtau, d->dVydtau, d->dVzdtau},
                     {d->betaVx, d->betaVy, d->betaVz}, {d->dtauVx, d->dtauVy, d->dtauVz}, {cnt.x, cnt.y, cnt.z}};
    for (int64_t itPH = 1; itPH <= 1000; itPH++) {
        itPH_done = itPH;
        if (rho_loop) JRX_TRY(jrx_compute_rhog(h, f->fz, rh, f->phase_c, f->T, f->P, nn, tdim, 3));      // update_ρg! :124
        JRX_TRY(dy3_strain_rp(h, s, a, true));
        a.rel = dp->lambda_relaxation_PH;
        JRX_TRY(dy3_stress(h, s, a, lin));
        hipLaunchKernelGGL(k_dy3_ph_residual, dy3_gc(a), dim3(256), 0, s, dy3_mom(a, d->dPpsi), f->Rx, f->Ry, f->Rz);
        DY3_LAUNCH(h);
        hipLaunchKernelGGL(k_dy3_ph_sums, dim3(nb), dim3(256), 0, s, (const double *)f->Rx, (const double *)f->Ry, (const double *)f->Rz, (const double *)f->RP, cnt.x, cnt.y,
                           cnt.z, cnt.c, h->d_partials);
        DY3_LAUNCH(h);
        JRX_TRY(dy3_read_sums(h, s, nb, 4));      // the host read of this Powell-Hestenes iteration
        double errV[3], e[4];
        for (int c = 0; c < 3; c++) errV[c] = sqrt(h->h_sums[c]) / sqrt(dofs[c]);
        errPt = sqrt(h->h_sums[3]) / sqrt(pdof);
        if (itPH == 1) { for (int c = 0; c < 3; c++) errV0[c] = errV[c] + EPS; errPt0 = errPt + EPS; }
        if (itPH == 2) errPt0 = errPt + EPS;
        for (int c = 0; c < 3; c++) e[c] = fmin(errV[c] / errV0[c], errV[c]);
        e[3] = fmin(errPt / errPt0, errPt);
        err = fmax(fmax(e[0], e[1]), fmax(e[2], e[3]));
        if (std::isnan(e[0]) || std::isnan(e[1]) || std::isnan(e[2]) || std::isnan(e[3])) err = NAN;
        if (dp->verbose_PH)
            printf("itPH = %02lld iter = %06lld iter/nx = %03lld, err = %1.3e - norm[R1=%1.3e %1.3e, R2=%1.3e %1.3e, R3=%1.3e %1.3e, Rp=%1.3e %1.3e] \n", (long long)itPH,
                   (long long)iter, (long long)(iter / nx), err, errV[0], errV[0] / errV0[0], errV[1], errV[1] / errV0[1], errV[2], errV[2] / errV0[2], errPt, errPt / errPt0);
        if (std::isnan(err)) { bad = jrx_fail(h, JRX_ERR_NAN, "NaN detected in outer loop"); break; }
        if (err > 1.0e10) { bad = jrx_fail(h, JRX_ERR_NAN, "Kaboom! Error > 1e10 in outer loop"); break; }
        if (err < dp->eps) break;
        if (err > err_min * 1.05) rel_drop = fmax(rel_drop * 0.1, 1.0e-3);
        if (err_min > err) err_min = err;
        const double eps_vel = err * rel_drop;
        int64_t itPT = 0;
        a.rel = dp->lambda_relaxation_DR;
        while (err > eps_vel && itPT <= dp->iterMax) {
            itPT++; iter++;
            const bool check = iter % dp->nout == 0;
            if (check) {      // pseudo-old residuals :191
                hipLaunchKernelGGL(k_copy6, dim3(256), dim3(256), 0, s, d->Rx0, (const double *)f->Rx, (i64)cnt.x, d->Ry0, (const double *)f->Ry, (i64)cnt.y, d->Rz0,
                                   (const double *)f->Rz, (i64)cnt.z, (double *)nullptr, (const double *)nullptr, (i64)0, (double *)nullptr, (const double *)nullptr, (i64)0,
                                   (double *)nullptr, (const double *)nullptr, (i64)0);
                DY3_LAUNCH(h);
            }
            JRX_TRY(dy3_strain_rp(h, s, a, true));
            JRX_TRY(dy3_stress(h, s, a, lin));
            hipLaunchKernelGGL(k_dy3_update, dy3_gc(a), dim3(256), 0, s, dy3_mom(a, d->P_num), dy3_upd(a));
            DY3_LAUNCH(h);
            // flow_bcs!: in the reference's pass order the first time and wherever the velocities can be observed (a check, the last iteration of a velocity solve);
            // in between, all faces in one launch, which agrees on every entry a stencil reads
            if (!bcs_applied || check || itPT > dp->iterMax) JRX_TRY(jrx3d_bcs(h, s, f->Vx, f->Vy, f->Vz, nx, ny, nz, p->free_slip, p->no_slip, 0));
            else JRX_TRY(jrx3d_bcs_faces(h, s, f->Vx, f->Vy, f->Vz, nx, ny, nz, p->free_slip, p->no_slip));
            bcs_applied = true;
            if (check) {
                hipLaunchKernelGGL(k_dy3_check_sums, dim3(nb), dim3(256), 0, s, chk, cnt.max, h->d_partials);
                DY3_LAUNCH(h);
                JRX_TRY(dy3_read_sums(h, s, nb, 9));      // the host read of these nout iterations
                const double *S = h->h_sums;
                double eV[3];
                for (int c = 0; c < 3; c++) eV[c] = sqrt(S[c]) / sqrt(dofs[c]);
                if (iter == dp->nout) errV00 = fmax(fmax(eV[0], eV[1]), eV[2]) + EPS;
                err = fmax(fmax(eV[0] / errV00, eV[1] / errV00), eV[2] / errV00);
                if (std::isnan(eV[0]) || std::isnan(eV[1]) || std::isnan(eV[2])) err = NAN;
                if (cont < res->cap) {
                    if (res->err_evo_tot) res->err_evo_tot[cont] = err;
                    if (res->err_evo_V) res->err_evo_V[cont] = err;
                    if (res->err_evo_P) res->err_evo_P[cont] = errPt / errPt0;
                    if (res->err_evo_it) res->err_evo_it[cont] = (double)iter;
                }
                cont++;
                if (std::isnan(err)) { bad = jrx_fail(h, JRX_ERR_NAN, "NaN detected in inner loop"); break; }
                if (dp->verbose_DR) printf("it = %lld, iter = %lld, err = %1.3e \n", (long long)itPT, (long long)iter, err);
                const double lmin = fabs((S[3] + S[4]) + S[5]) / ((S[6] + S[7]) + S[8]);      // compute_λminV! :359-365
                const double cV = 2 * sqrt(lmin) * dp->c_fact;
                hipLaunchKernelGGL(k_dy3_fill3, dim3(dy3_g1(cnt.max)), dim3(256), 0, s, d->cVx, cnt.x, d->cVy, cnt.y, d->cVz, cnt.z, cV);
                DY3_LAUNCH(h);
                JRX_TRY(dy3_gershgorin(h, s, a));
                JRX_TRY(dy3_dtau(h, s, a, dp->CFL, true));
            }
        }
        if (bad != JRX_OK) break;
        JRX_TRY(dy3_strain_rp(h, s, a, false));      // update pressure :263-264
        hipLaunchKernelGGL(k_dy3_add_P, dim3(dy3_g1(cnt.c)), dim3(256), 0, s, f->P, (const double *)d->gamma_eff, (const double *)f->RP, cnt.c);
        DY3_LAUNCH(h);
        if (iter > dp->total_iterMax) break;
    }
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    if (bad == JRX_OK) {      // epilogue :269-290; copy_stress_vertices!(Val(3)) has nothing to copy: no vertex-normal stresses are kept in 3D
        hipLaunchKernelGGL(k_dy3_epilogue, dy3_gv(a), dim3(256), 0, s, a);
        DY3_LAUNCH(h);
        JRX_TRY((jrx3d_copy_old_stresses<256>(h, s, f, nx, ny, nz)));
        h->stat_dyrel_launches += 2;
    }
    JRX_HIP(h, hipStreamSynchronize(s));
    float ms = 0.f;
    JRX_HIP(h, hipEventElapsedTime(&ms, h->ev[6], h->ev[7]));
    res->iter = iter; res->itPH = itPH_done;
    res->nchecks = cont < res->cap ? cont : res->cap;
    res->time_s = ms * 1e-3;
    return bad;
}

}   // extern "C"
