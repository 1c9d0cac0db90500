// dyrel_common.hpp -- what dyrel2d.hip and dyrel3d.hip share on the device and around launches, for ND = 2 or 3 velocity components: the fixed-order sums, the
// check-time kernels over the per-component arrays of the DYREL struct (DyDof), DYREL! and the solve loop (dy_solve).  The stencil kernels, what an entry point
// refuses and the prologue of a solve stay with each file; the loop's error bookkeeping is dyrel_conv.hpp's.
//
// Reference (PTsolvers/JustRelax.jl): src/DYREL/solver.jl:117-290 (the loop of _solve_DYREL!), constructors.jl:178-190 (DYREL!), :230-254
// (compute_bulk_viscosity_and_penalty!), velocity_kernels.jl:625-658 (compute_dV!, update_cV!), Gershgorin.jl:171-310 (update_α_β!, update_dτV_α_β!).
//
// dy_solve<O> is instantiated once per file with that file's launch object O, which has: ND; MAXBLK (the cap on the blocks of a sum); Args (the kernels' argument
// struct, with f, d, rh, nx, rel); h, s, a (the handle, the stream, an Args); dofs, pdof (velocity_dofs, pressure_dof); cells(), dof(); and the launches strain_rp,
// stress, ph_residual, copy_old_residual, update_V (with its flow_bcs!), gershgorin, rhog, epilogue (with its old-stress copy).  Dispatch is static.
// Fixed, because they fix the summation order: block size 256, the grid-stride loop with the components in order, partial rows of 4 ND, MAXBLK.
// fma only in k_dy_dtau (the reference's @muladd).
#pragma once
#include <initializer_list>
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_material.hpp"
#include "dyrel_conv.hpp"

namespace {

inline bool dy_has(std::initializer_list<const void *> req)
{
    for (const void *q : req)
        if (!q) return false;
    return true;
}
#define DY_REQ(h, what, ...) \
    if (!dy_has({__VA_ARGS__})) return jrx_fail(h, JRX_ERR_ARG, "%s: a required field pointer is NULL", what)
#define DY_LAUNCH(h) \
    do { (h)->stat_dyrel_launches++; JRX_LAUNCH_CHECK(h); } while (0)

// the per-component arrays of the DYREL struct (types.jl:24-59) with the momentum residual R of StokesArrays and the node count of each component
template <int ND>
struct DyDof {
    double *R[ND], *R0[ND], *D[ND], *lmax[ND], *dVdtau[ND], *dtau[ND], *dV[ND], *beta[ND], *cV[ND], *alpha[ND];
    int n[ND], nmax;
};

inline unsigned dy_g1(int n) { return (unsigned)((n + 255) / 256); }
// the blocks of a sum: partial rows of 4 ND, so MAXBLK rows must fit the kMaxRedBlocks rows of 4 of the handle's scratch
template <class O>
int dy_nblk(const O &o)
{
    static_assert(O::MAXBLK * 4 * O::ND <= kMaxRedBlocks * 4, "the reduction scratch holds the partial rows");
    const unsigned g = (dy_g1(o.cells()) + 7) / 8;
    return (int)(g < 1 ? 1 : (g > (unsigned)O::MAXBLK ? (unsigned)O::MAXBLK : g));
}

// fixed-order two-stage sums, no atomics: wave shuffle -> the four waves of a block -> one partial row of NS per block -> k_dy_sum_final in one block
template <int NS>
__device__ __forceinline__ void dy_block_store(const double s[NS], const int ns, double *__restrict__ partials)
{
    __shared__ double sm[NS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < ns; c++) {
        const double w = wave_sum(s[c]);
        if (lane == 0) sm[c][wave] = w;
    }
    __syncthreads();
    if ((int)threadIdx.x < NS) {
        const int c = threadIdx.x;
        partials[blockIdx.x * NS + c] = c < ns ? (sm[c][0] + sm[c][1]) + (sm[c][2] + sm[c][3]) : 0.0;
    }
}
template <int NS>
__global__ __launch_bounds__(256) void k_dy_sum_final(const double *__restrict__ partials, const int nblocks, double *__restrict__ out)
{
    __shared__ double sm[NS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NS; c++) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += partials[b * NS + c];
        s = wave_sum(s);
        if (lane == 0) sm[c][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int c = threadIdx.x;
        out[c] = (sm[c][0] + sm[c][1]) + (sm[c][2] + sm[c][3]);
    }
}
// Σ η and the count over the finite entries
template <int NS>
__global__ __launch_bounds__(256) void k_dy_eta_sum(const double *__restrict__ eta, const int n, double *__restrict__ partials)
{
    double s[NS] = {};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const double e = eta[t];
        if (!isinf(e)) { s[0] += e; s[1] += 1.0; }
    }
    dy_block_store<NS>(s, 2, partials);
}
// compute_bulk_viscosity_and_penalty! (constructors.jl:237-254) over n cells; eta_mean = mean(η[.!isinf.(η)]) is sums[0] / sums[1] of k_dy_eta_sum
template <class A>
__global__ __launch_bounds__(256) void k_dy_bulk(const A a, const int n, const double *__restrict__ sums, const double gamma_fact)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double eta_mean = sums[0] / sums[1];
    const double Kbdt = ratio_avg(a.rh.Kb, a.f.phase_c + a.rh.nphase * t, a.rh.nphase) * a.dt;
    a.d.etab[t] = Kbdt;
    const double e = a.f.eta[t];
    const double g_num = gamma_fact * (isinf(e) ? eta_mean : e);
    const double g_phy = isinf(Kbdt) ? g_num : Kbdt;
    a.d.gamma_eff[t] = g_phy * g_num / (g_phy + g_num);
}
// the Powell-Hestenes norms (solver.jl:151-152): Σ R_c² per component, Σ RP² over the whole arrays
template <int ND>
__global__ __launch_bounds__(256) void k_dy_ph_sums(const DyDof<ND> d, const double *__restrict__ RP, const int n, double *__restrict__ partials)
{
    double s[4 * ND] = {};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < ND; c++)
            if (t < d.n[c]) { const double v = d.R[c][t]; s[c] += v * v; }
        const double v = RP[t];
        s[ND] += v * v;
    }
    dy_block_store<4 * ND>(s, ND + 1, partials);
}
// the residual check of the inner loop (solver.jl:231,251, :359-365): compute_dV!, then per component Σ (D R)², Σ dV (R - R0), Σ dV²
template <int ND>
__global__ __launch_bounds__(256) void k_dy_check_sums(const DyDof<ND> d, double *__restrict__ partials)
{
    double s[4 * ND] = {};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < d.nmax; t += gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < ND; c++) {
            if (t >= d.n[c]) continue;
            const double R = d.R[c][t], DR = d.D[c][t] * R, dV = d.dVdtau[c][t] * d.beta[c][t] * d.dtau[c][t];
            d.dV[c][t] = dV;
            s[c] += DR * DR; s[ND + c] += dV * (R - d.R0[c][t]); s[2 * ND + c] += dV * dV;
        }
    }
    dy_block_store<4 * ND>(s, 3 * ND, partials);
}
// update_cV! (velocity_kernels.jl:642-654)
template <int ND>
__global__ __launch_bounds__(256) void k_dy_fill(const DyDof<ND> d, const double v)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int c = 0; c < ND; c++)
        if (t < d.n[c]) d.cV[c][t] = v;
}
// _update_dτV_α_β! (Gershgorin.jl:229-247, 290-310; DTAU) / _update_α_β! (:182-198): the reference's @muladd is the two fma here
template <int ND, bool DTAU>
__global__ __launch_bounds__(256) void k_dy_dtau(const DyDof<ND> d, const double CFL)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int c = 0; c < ND; c++) {
        if (t >= d.n[c]) continue;
        double x = d.dtau[c][t];
        if (DTAU) { x = 2 / sqrt(d.lmax[c][t]) * CFL; d.dtau[c][t] = x; }
        const double cv = d.cV[c][t], den = fma(cv, x, 2.0);
        d.beta[c][t] = 2 * x / den;
        d.alpha[c][t] = fma(-cv, x, 2.0) / den;
    }
}
// @. P += γ_eff * RP (solver.jl:264)
__global__ __launch_bounds__(256) void k_dy_add_P(double *__restrict__ P, const double *__restrict__ gam, const double *__restrict__ RP, const int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) P[t] = P[t] + gam[t] * RP[t];
}

// the sums of one reduction kernel, read on the host: the one synchronisation of a check
template <int NS>
jrx_status dy_read_sums(jrx_handle *h, hipStream_t s, int nb, int count)
{
    hipLaunchKernelGGL(k_dy_sum_final<NS>, dim3(1), dim3(256), 0, s, (const double *)h->d_partials, nb, h->d_sums);
    DY_LAUNCH(h);
    JRX_HIP(h, hipMemcpyAsync(h->h_sums, h->d_sums, count * sizeof(double), hipMemcpyDeviceToHost, s));
    JRX_HIP(h, hipStreamSynchronize(s));
    return JRX_OK;
}
template <class O>
jrx_status dy_dtau(const O &o, double CFL, bool from_lmax)
{
    const DyDof<O::ND> q = o.dof();
    if (from_lmax) hipLaunchKernelGGL((k_dy_dtau<O::ND, true>), dim3(dy_g1(q.nmax)), dim3(256), 0, o.s, q, CFL);
    else hipLaunchKernelGGL((k_dy_dtau<O::ND, false>), dim3(dy_g1(q.nmax)), dim3(256), 0, o.s, q, CFL);
    DY_LAUNCH(o.h);
    return JRX_OK;
}
template <class O>
jrx_status dy_bulk(const O &o, double gamma_fact)
{
    constexpr int NS = 4 * O::ND;
    const int nb = dy_nblk(o), n = o.cells();
    hipLaunchKernelGGL(k_dy_eta_sum<NS>, dim3(nb), dim3(256), 0, o.s, (const double *)o.a.f.eta, n, o.h->d_partials);
    DY_LAUNCH(o.h);
    hipLaunchKernelGGL(k_dy_sum_final<NS>, dim3(1), dim3(256), 0, o.s, (const double *)o.h->d_partials, nb, o.h->d_sums);
    DY_LAUNCH(o.h);
    hipLaunchKernelGGL(k_dy_bulk<typename O::Args>, dim3(dy_g1(n)), dim3(256), 0, o.s, o.a, n, (const double *)o.h->d_sums, gamma_fact);
    DY_LAUNCH(o.h);
    return JRX_OK;
}
// DYREL! (constructors.jl:178-190)
template <class O>
jrx_status dy_init(const O &o, double CFL, double gamma_fact)
{
    JRX_TRY(dy_bulk(o, gamma_fact));
    JRX_TRY(o.gershgorin());
    return dy_dtau(o, CFL, true);
}

// _solve_DYREL! from compute_ρg! on (solver.jl:118-290); the caller has checked the arguments, run the prologue :86-95, recorded h->ev[6] and computed the viscosity
template <class O>
jrx_status dy_solve(O &o, const jrx_dyrel2d_params *dp, jrx_dyrel2d_result *res)
{
    constexpr int ND = O::ND, NS = 4 * ND;
    jrx_handle *h = o.h;
    hipStream_t s = o.s;
    const jrx_rheology *rh = &o.a.rh;
    const bool lin = dp->linear_viscosity != 0;
    const int nb = dy_nblk(o), n = o.cells();
    const DyDof<ND> q = o.dof();
    if (rh->has_density) JRX_TRY(o.rhog());      // compute_ρg!(ρg[end], ...), DYREL! :118-119
    JRX_TRY(dy_init(o, dp->CFL, dp->gamma_fact));
    const bool rho_loop = rh->has_density && !mat_density_is_constant(rh);

    DyrelConv<ND> conv(dp, res, o.dofs, o.pdof);
    int64_t iter = 0, itPH_done = 0;
    jrx_status bad = JRX_OK;
    for (int64_t itPH = 1; itPH <= 1000; itPH++) {
        itPH_done = itPH;
        if (rho_loop) JRX_TRY(o.rhog());      // update_ρg! :124
        JRX_TRY(o.strain_rp(true));
        o.a.rel = dp->lambda_relaxation_PH;
        JRX_TRY(o.stress(lin));
        JRX_TRY(o.ph_residual());
        hipLaunchKernelGGL(k_dy_ph_sums<ND>, dim3(nb), dim3(256), 0, s, q, (const double *)o.a.f.RP, n, h->d_partials);
        DY_LAUNCH(h);
        JRX_TRY(dy_read_sums<NS>(h, s, nb, ND + 1));      // the host read of this Powell-Hestenes iteration
        const DyVerdict v = conv.outer(itPH, iter, o.a.nx, h->h_sums);
        if (v == DY_NAN) { bad = jrx_fail(h, JRX_ERR_NAN, "NaN detected in outer loop"); break; }
        if (v == DY_KABOOM) { bad = jrx_fail(h, JRX_ERR_NAN, "Kaboom! Error > 1e10 in outer loop"); break; }
        if (v == DY_CONVERGED) break;
        int64_t itPT = 0;
        o.a.rel = dp->lambda_relaxation_DR;
        while (conv.err() > conv.eps_vel() && itPT <= dp->iterMax) {
            itPT++; iter++;
            const bool check = iter % dp->nout == 0;
            if (check) JRX_TRY(o.copy_old_residual());      // pseudo-old residuals :191
            JRX_TRY(o.strain_rp(true));
            JRX_TRY(o.stress(lin));
            JRX_TRY(o.update_V(check, itPT > dp->iterMax));
            if (check) {
                hipLaunchKernelGGL(k_dy_check_sums<ND>, dim3(nb), dim3(256), 0, s, q, h->d_partials);
                DY_LAUNCH(h);
                JRX_TRY(dy_read_sums<NS>(h, s, nb, 3 * ND));      // the host read of these nout iterations
                double cV;
                if (!conv.inner(itPT, iter, h->h_sums, &cV)) { bad = jrx_fail(h, JRX_ERR_NAN, "NaN detected in inner loop"); break; }
                hipLaunchKernelGGL(k_dy_fill<ND>, dim3(dy_g1(q.nmax)), dim3(256), 0, s, q, cV);
                DY_LAUNCH(h);
                JRX_TRY(o.gershgorin());
                JRX_TRY(dy_dtau(o, dp->CFL, true));
            }
        }
        if (bad != JRX_OK) break;
        JRX_TRY(o.strain_rp(false));      // update pressure :263-264
        hipLaunchKernelGGL(k_dy_add_P, dim3(dy_g1(n)), dim3(256), 0, s, o.a.f.P, (const double *)o.a.d.gamma_eff, (const double *)o.a.f.RP, n);
        DY_LAUNCH(h);
        if (iter > dp->total_iterMax) break;
    }
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    if (bad == JRX_OK) JRX_TRY(o.epilogue());      // :269-290
    JRX_HIP(h, hipStreamSynchronize(s));
    float ms = 0.f;
    JRX_HIP(h, hipEventElapsedTime(&ms, h->ev[6], h->ev[7]));
    conv.finish(iter, itPH_done, ms);
    return bad;
}

}   // namespace
