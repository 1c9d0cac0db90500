// dyrel3d.hip -- 3D DYREL (self-tuned dynamic relaxation inside Powell-Hestenes pressure iterations) for gfx950: kernels, per-kernel entry points, driver.
//
// Reference (PTsolvers/JustRelax.jl).  Restated: src/DYREL/constructors.jl:61-111 (the 3D allocator), solver.jl:44-294 (_solve_DYREL!; here its prologue :86-117,
// the loop is dyrel_common.hpp's), :329-357 (dyrel_fields(Val(3)), velocity_dofs, pressure_dof), velocity_kernels.jl:242-322 (compute_∇V_strain_rate_RP! 3D), :441-477
// (compute_PH_residual_V! 3D), :660-663 (damped_update_V), :729-828 (compute_DR_residual_update_V! 3D), stress_kernels.jl:224-315 (the local law, dyrel_local.hpp).
// Shared with dyrel2d.hip: the sums, the check-time kernels, DYREL! and the solve loop (dyrel_common.hpp), its error bookkeeping (dyrel_conv.hpp).
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
// edges average τ_o, ε, P, EII_pl, which it never writes.  32-bit element offsets (the extents are checked against 2^31).
#include "dyrel_common.hpp"
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

// the launches of this file's kernels on the handle's stream: what the entry points below call, and the launch object of dy_solve (dyrel_common.hpp)
struct Dy3 {
    typedef Dy3Args Args;
    static constexpr int ND = 3, MAXBLK = 512;      // partial rows of 12: 512 rows fit kMaxRedBlocks rows of 4
    jrx_handle *h;
    hipStream_t s;
    Dy3Args a;
    double dofs[3], pdof;      // velocity_dofs(Val(3)), pressure_dof (solver.jl:349-357)
    bool bcs_applied = false;      // flow_bcs! has run in the reference's pass order on V since the solve began

    Dy3(jrx_handle *h_, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p) : h(h_), s(h_->stream)
    {
        memset(&a, 0, sizeof(a));
        a.f = *f; a.d = *d;
        if (rh) a.rh = *rh;
        a._dx = p->_dx; a._dy = p->_dy; a._dz = p->_dz; a.dt = p->dt;
        a.nx = (int)p->nx; a.ny = (int)p->ny; a.nz = (int)p->nz;
        a.fs = p->free_slip; a.ns = p->no_slip;
        a.tg = p->T_ghosted != 0;
        a.rel = 1.0; a.nu = 1.0e-2; a.cut_lo = -INFINITY; a.cut_hi = INFINITY;
        dofs[0] = (double)((p->nxg - 2) * (p->nyg - 1) * (p->nzg - 1)); dofs[1] = (double)((p->nxg - 1) * (p->nyg - 2) * (p->nzg - 1));
        dofs[2] = (double)((p->nxg - 1) * (p->nyg - 1) * (p->nzg - 2));
        pdof = (double)(p->nxg * p->nyg * p->nzg);
    }
    int cells() const { return a.nx * a.ny * a.nz; }
    dim3 gv() const { return DY3_GRID(a.nx + 1, a.ny + 1, a.nz + 1); }
    dim3 gc() const { return DY3_GRID(a.nx, a.ny, a.nz); }
    Dy3Mom mom(const double *th) const
    {
        return Dy3Mom{a.f.P, th, a.f.txx, a.f.tyy, a.f.tzz, a.f.tyz, a.f.txz, a.f.txy, a.f.fx, a.f.fy, a.f.fz, a._dx, a._dy, a._dz, a.nx, a.ny, a.nz};
    }
    Dy3Upd upd() const
    {
        const jrx_dyrel3d_fields &d = a.d;
        return Dy3Upd{{a.f.Rx, a.f.Ry, a.f.Rz}, {a.f.Vx, a.f.Vy, a.f.Vz}, {d.dVxdtau, d.dVydtau, d.dVzdtau}, {d.Dx, d.Dy, d.Dz}, {d.alphaVx, d.alphaVy, d.alphaVz},
                      {d.betaVx, d.betaVy, d.betaVz}, {d.dtauVx, d.dtauVy, d.dtauVz}};
    }
    DyDof<3> dof() const
    {
        const jrx_dyrel3d_fields &d = a.d;
        const int nxn = (a.nx - 1) * a.ny * a.nz, nyn = a.nx * (a.ny - 1) * a.nz, nzn = a.nx * a.ny * (a.nz - 1), nxy = nxn > nyn ? nxn : nyn;
        return DyDof<3>{{a.f.Rx, a.f.Ry, a.f.Rz}, {d.Rx0, d.Ry0, d.Rz0}, {d.Dx, d.Dy, d.Dz}, {d.lmaxVx, d.lmaxVy, d.lmaxVz}, {d.dVxdtau, d.dVydtau, d.dVzdtau},
                        {d.dtauVx, d.dtauVy, d.dtauVz}, {d.dVx, d.dVy, d.dVz}, {d.betaVx, d.betaVy, d.betaVz}, {d.cVx, d.cVy, d.cVz}, {d.alphaVx, d.alphaVy, d.alphaVz},
                        {nxn, nyn, nzn}, nzn > nxy ? nzn : nxy};
    }

    jrx_status strain_rp(bool strain) const
    {
        const jrx_vep3d_fields &f = a.f;
        if (strain) hipLaunchKernelGGL(k_dy3_strain_rp<true>, gv(), dim3(256), 0, s, f.exx, f.eyy, f.ezz, f.eyz, f.exz, f.exy, (const double *)f.Vx, (const double *)f.Vy,
                                       (const double *)f.Vz, f.RP, (const double *)f.P, (const double *)f.P0, (const double *)f.Q, (const double *)a.d.etab, a._dx, a._dy, a._dz,
                                       a.dt, a.nx, a.ny, a.nz);
        else hipLaunchKernelGGL(k_dy3_strain_rp<false>, gv(), dim3(256), 0, s, f.exx, f.eyy, f.ezz, f.eyz, f.exz, f.exy, (const double *)f.Vx, (const double *)f.Vy,
                                (const double *)f.Vz, f.RP, (const double *)f.P, (const double *)f.P0, (const double *)f.Q, (const double *)a.d.etab, a._dx, a._dy, a._dz, a.dt,
                                a.nx, a.ny, a.nz);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    template <bool SOFT, bool LIN>
    jrx_status stress_t() const
    {
        hipLaunchKernelGGL((k_dy3_stress<SOFT, LIN, 7>), gv(), dim3(256), 0, s, a);
        DY_LAUNCH(h);
        hipLaunchKernelGGL((k_dy3_stress<SOFT, LIN, 8>), gc(), dim3(256), 0, s, a);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status stress(bool lin) const
    {
        if (mat_has_softening(&a.rh)) return lin ? stress_t<true, true>() : stress_t<true, false>();
        return lin ? stress_t<false, true>() : stress_t<false, false>();
    }
    jrx_status ph_residual() const
    {
        hipLaunchKernelGGL(k_dy3_ph_residual, gc(), dim3(256), 0, s, mom(a.d.dPpsi), a.f.Rx, a.f.Ry, a.f.Rz);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status copy_old_residual() const
    {
        const DyDof<3> q = dof();
        hipLaunchKernelGGL(k_copy6, dim3(256), dim3(256), 0, s, q.R0[0], (const double *)q.R[0], (i64)q.n[0], q.R0[1], (const double *)q.R[1], (i64)q.n[1], q.R0[2],
                           (const double *)q.R[2], (i64)q.n[2], (double *)nullptr, (const double *)nullptr, (i64)0, (double *)nullptr, (const double *)nullptr, (i64)0,
                           (double *)nullptr, (const double *)nullptr, (i64)0);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status update() const
    {
        hipLaunchKernelGGL(k_dy3_update, gc(), dim3(256), 0, s, mom(a.d.P_num), upd());
        DY_LAUNCH(h);
        return JRX_OK;
    }
    // flow_bcs!: in the reference's pass order the first time and wherever the velocities can be observed (a check, the last iteration of a velocity solve);
    // in between, all faces in one launch, which agrees on every entry a stencil reads
    jrx_status update_V(bool check, bool last)
    {
        JRX_TRY(update());
        if (!bcs_applied || check || last) JRX_TRY(jrx3d_bcs(h, s, a.f.Vx, a.f.Vy, a.f.Vz, a.nx, a.ny, a.nz, a.fs, a.ns, 0));
        else JRX_TRY(jrx3d_bcs_faces(h, s, a.f.Vx, a.f.Vy, a.f.Vz, a.nx, a.ny, a.nz, a.fs, a.ns));
        bcs_applied = true;
        return JRX_OK;
    }
    jrx_status gershgorin() const
    {
        hipLaunchKernelGGL(k_dy3_gershgorin, gc(), dim3(256), 0, s, a);
        DY_LAUNCH(h);
        return JRX_OK;
    }
    jrx_status rhog() const      // ρg[end] = ρg z
    {
        const int64_t nn[3] = {a.nx, a.ny, a.nz}, tdim[3] = {a.tg ? a.nx + 2 : a.nx, a.tg ? a.ny + 2 : a.ny, a.tg ? a.nz + 2 : a.nz};
        return jrx_compute_rhog(h, a.f.fz, &a.rh, a.f.phase_c, a.f.T, a.f.P, nn, tdim, 3);
    }
    jrx_status epilogue() const      // copy_stress_vertices!(Val(3)) has nothing to copy: no vertex-normal stresses are kept in 3D
    {
        hipLaunchKernelGGL(k_dy3_epilogue, gv(), dim3(256), 0, s, a);
        DY_LAUNCH(h);
        JRX_TRY((jrx3d_copy_old_stresses<256>(h, s, &a.f, a.nx, a.ny, a.nz)));
        h->stat_dyrel_launches += 2;
        return JRX_OK;
    }
};

#define DY3_FIELDS_STRESS(f, d)                                                                                                                                    \
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
    DY_REQ(h, "compute_∇V_strain_rate_RP! 3D", f->exx, f->eyy, f->ezz, f->eyz, f->exz, f->exy, f->Vx, f->Vy, f->Vz, f->RP, f->P, f->P0, f->Q, d->etab);
    JRX_TRY(Dy3(h, f, d, nullptr, p).strain_rp(do_strain_rate != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_stress_viscosity(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p,
                                        const jrx_dyrel2d_params *dp, double lambda_relaxation)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, rh, p));
    if (!rh || !dp) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY_REQ(h, "compute_stress_viscosity_DRYEL! 3D", DY3_FIELDS_STRESS(f, d));
    Dy3 o(h, f, d, rh, p);
    o.a.rel = lambda_relaxation; o.a.nu = dp->viscosity_relaxation; o.a.cut_lo = dp->cutoff_lo; o.a.cut_hi = dp->cutoff_hi;
    JRX_TRY(o.stress(dp->linear_viscosity != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_PH_residual(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, nullptr, p));
    DY_REQ(h, "compute_PH_residual_V! 3D", DY3_FIELDS_MOM(f), d->dPpsi);
    JRX_TRY(Dy3(h, f, d, nullptr, p).ph_residual());
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_DR_residual_update_V(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, nullptr, p));
    DY_REQ(h, "compute_DR_residual_update_V! 3D", DY3_FIELDS_MOM(f), f->Vx, f->Vy, f->Vz, d->P_num, d->Dx, d->Dy, d->Dz, d->dVxdtau, d->dVydtau, d->dVzdtau, d->alphaVx,
           d->alphaVy, d->alphaVz, d->betaVx, d->betaVy, d->betaVz, d->dtauVx, d->dtauVy, d->dtauVz);
    JRX_TRY(Dy3(h, f, d, nullptr, p).update());
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_gershgorin(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, rh, p));
    if (!rh) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY_REQ(h, "the 3D Gershgorin estimate", f->eta, f->phase_c, f->phase_yz, f->phase_xz, f->phase_xy, d->gamma_eff, d->Dx, d->Dy, d->Dz, d->lmaxVx, d->lmaxVy, d->lmaxVz);
    JRX_TRY(Dy3(h, f, d, rh, p).gershgorin());
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_update_dtauV_alpha_beta(jrx_handle *h, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p, double CFL, int32_t from_lambda_max)
{
    jrx_vep3d_fields none;
    memset(&none, 0, sizeof(none));
    JRX_TRY(dy3_check(h, &none, d, nullptr, nullptr, p));
    DY_REQ(h, "update_dτV_α_β! 3D", d->dtauVx, d->dtauVy, d->dtauVz, d->betaVx, d->betaVy, d->betaVz, d->alphaVx, d->alphaVy, d->alphaVz, d->cVx, d->cVy, d->cVz, d->lmaxVx,
           d->lmaxVy, d->lmaxVz);
    JRX_TRY(dy_dtau(Dy3(h, &none, d, nullptr, p), CFL, from_lambda_max != 0));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_bulk_viscosity_and_penalty(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh,
                                                  const jrx_vep3d_params *p, double gamma_fact)
{
    JRX_TRY(dy3_check(h, f, d, nullptr, rh, p));
    if (!rh) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY_REQ(h, "compute_bulk_viscosity_and_penalty! 3D", f->eta, f->phase_c, d->etab, d->gamma_eff);
    JRX_TRY(dy_bulk(Dy3(h, f, d, rh, p), gamma_fact));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_init(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                            const jrx_vep3d_params *p, const jrx_dyrel2d_params *dp)
{
    JRX_TRY(dy3_check(h, f, d, phi, rh, p));
    if (!rh || !dp) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    DY_REQ(h, "DYREL! 3D", f->eta, f->phase_c, f->phase_yz, f->phase_xz, f->phase_xy, d->gamma_eff, d->etab, DY3_FIELDS_DAMP(d));
    JRX_TRY(dy_init(Dy3(h, f, d, rh, p), dp->CFL, dp->gamma_fact));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_dyrel3d_solve(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                             const jrx_vep3d_params *p, const jrx_dyrel2d_params *dp, jrx_dyrel2d_result *res)
{
    JRX_TRY(dy3_check(h, f, d, phi, rh, p));
    if (!rh || !dp || !res) return jrx_fail(h, JRX_ERR_ARG, "DYREL 3D: null argument");
    if (dp->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    DY_REQ(h, "solve_DYREL! 3D", DY3_FIELDS_STRESS(f, d), DY3_FIELDS_MOM(f), DY3_FIELDS_DAMP(d), f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Vz, f->eplyz_c, f->eplxz_c,
           f->eplxy_c, f->EVol_pl, d->etab);
    if (mat_viscosity_reads_invariant(rh) && !(f->eyz_c && f->exz_c && f->exy_c)) return jrx_fail(h, JRX_ERR_ARG, "a power-law creep needs the centre shear strain rates for compute_viscosity!");
    Dy3 o(h, f, d, rh, p);
    o.a.nu = dp->viscosity_relaxation; o.a.cut_lo = dp->cutoff_lo; o.a.cut_hi = dp->cutoff_hi;
    hipStream_t s = o.s;
    const size_t n = (size_t)o.cells();
    const EdgeN ne = edge_counts(o.a.nx, o.a.ny, o.a.nz);

    // solver.jl:86-95: P0 <- P, @tensor_center(ε_pl) = 0, λ = λv = 0
    JRX_HIP(h, hipMemcpyAsync(f->P0, f->P, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (double *q : {f->eplxx, f->eplyy, f->eplzz, f->eplyz_c, f->eplxz_c, f->eplxy_c, d->lambda}) JRX_HIP(h, hipMemsetAsync(q, 0, n * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_yz, 0, (size_t)ne.yz * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_xz, 0, (size_t)ne.xz * sizeof(double), s));
    JRX_HIP(h, hipMemsetAsync(d->lambda_xy, 0, (size_t)ne.xy * sizeof(double), s));
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    {   // :117: compute_viscosity! (relaxation 1, the strain-rate invariant)
        jrx_vep3d_params pv = *p;
        pv.cutoff_lo = dp->cutoff_lo; pv.cutoff_hi = dp->cutoff_hi;
        JRX_TRY(jrx_vep3d_compute_viscosity(h, f, rh, &pv, 1.0));
    }
    return dy_solve(o, dp, res);
}

}   // extern "C"
