// thermal_common.hpp -- the pseudo-transient loop thermal2d.hip and thermal3d.hip share (heat_solve) and update_ΔT!.  The stencil kernels, what an entry point
// refuses, the forms that fuse and the tile dispatch stay with each file; which iterations are observed is heat_plan.hpp's.
//
// Reference (PTsolvers/JustRelax.jl): src/thermal_diffusion/DiffusionPT_solver.jl:91-149 (array form) and :221-305 (rheology / phase-ratio form).
//
// heat_solve<O> is instantiated per file and phase type with that file's launch object O (Heat2<PHT>, Heat3<PHT>).  A set is (T, qT) and, where it swaps too, θr_dτ:
// set 0 the caller's arrays, set 1 the library's.  O has: PH (phase-ratio form); SUB_BLOCKS (the grid of update_ΔT!); h, a (the handle; the kernels' argument
// struct with t and p); n[3] (cells per direction, 1 for a missing one); nodes() (entries of T); fusable (unobserved iterations run as one launch from a set into
// the other); and
//   second_set()          make set 1, with the ghosts of T that no BC rewrites
//   fused(c)              one iteration in one launch from set c into the other
//   two_kernels(c, o, w)  compute_flux! + update_T! + thermal_bcs! in place on set c; o: an observed iteration; w: update_T! writes the next PT coefficients
//   residual(c)           check_res! on set c
//   refresh_pt(c)         update_pt_thermal_arrays! from the T of set c (phase-ratio form)
//   copy_back()           set 1 into the caller's arrays
//   graphable()           runs of unobserved iterations may replay as graphs
//   graph_iteration(c)    what one iteration of such a graph enqueues
// Dispatch is static.
#pragma once
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_thermal_phases.hpp"
#include "heat_plan.hpp"

namespace {

__global__ __launch_bounds__(256) void k_sub(double *__restrict__ d, const double *__restrict__ a, const double *__restrict__ b, i64 n)
{
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (i64)gridDim.x * blockDim.x) d[t] = a[t] - b[t];
}

// heatdiffusion_PT! from `@copy thermal.Told thermal.T` on; the caller has checked the arguments
template <class O>
jrx_status heat_solve(O &o, int64_t *iter_count, double *norm_ResT, int64_t cap, int64_t *nnorms)
{
    constexpr int GIT = heat_plan::kGraphIters;
    jrx_handle *h = o.h;
    hipStream_t s = h->stream;
    const auto p = o.a.p;
    const auto t = o.a.t;      // the caller's arrays (o.a.t follows the current set)
    if (p.nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    const i64 n = (i64)o.n[0] * o.n[1] * o.n[2];
    const double sq = 1.0 / sqrt((double)n);
    JRX_HIP(h, hipMemcpyAsync(t.Told, t.T, (size_t)o.nodes() * sizeof(double), hipMemcpyDeviceToDevice, s));   // @copy thermal.Told thermal.T
    // iterations nobody observes: one fused launch, ping-pong between the caller's set and a library-owned one (option "thermal_fused"); observed ones (a check
    // follows, or the last) run the two kernels in place on the current set
    if (o.fusable) JRX_TRY(o.second_set());
    int cur = 0;
    int64_t iter = 0, cnt = 0;
    double err = 2 * p.eps;
    bool pt_fresh = false;      // phase-ratio form: θr_dτ, dτ_ρ belong to the current T
    // Runs of unobserved iterations replay as captured graphs of GIT iterations: on launch-bound grids the gap between dependent launches is shorter inside a graph
    // (scripts/graph_probe.hip: 4.6 vs 5.7 - 6.1 us per pair of short kernels; profiles/r03_small_grids_graphs.txt).  One graph per current set, built on first use,
    // released on every exit path; option "loop_graphs" = 0, or a capture the runtime refuses, keeps plain launches.
    GraphExecs gexec;
    bool graphs = h->loop_graphs && o.graphable();
    while (err > p.eps && iter < p.iterMax) {
        // the two kernels of the phase-ratio form replay only while update_T! keeps the PT coefficients fresh; its fused form refreshes them ahead of a replay
        if (graphs && (!O::PH || pt_fresh || o.fusable) && heat_plan::unobserved_run(iter, p.nout, p.iterMax) >= GIT) {
            if (!gexec[cur]) {
                JRX_TRY(jrx_capture_graph(s, &gexec[cur], [&]() -> jrx_status {
                    for (int q = 0, c = cur; q < GIT; q++, c ^= (int)o.fusable) JRX_TRY(o.graph_iteration(c));
                    return JRX_OK;
                }));
                if (!gexec[cur]) graphs = false;
            }
            if (gexec[cur]) {
                if (O::PH && !pt_fresh) JRX_TRY(o.refresh_pt(cur));
                for (int64_t run = heat_plan::unobserved_run(iter, p.nout, p.iterMax); run >= GIT; run -= GIT) {
                    JRX_HIP(h, hipGraphLaunch(gexec[cur], s));
                    iter += GIT;
                    if (o.fusable) h->stat_thermal_fused += GIT;
                    h->stat_graph_replays++;
                }
                pt_fresh = O::PH;
                continue;
            }
        }
        const bool observed = heat_plan::observes_next(iter, p.nout, p.iterMax);
        if constexpr (O::PH) {      // update_pt_thermal_arrays!(pt_thermal, phase, rheology, args, _dt) -- DiffusionPT_solver.jl:233-234
            // on unobserved iterations update_T! writes the coefficients of the next iteration itself (same values: they depend on the cell's own new T
            // only); observed iterations leave pt_thermal as the reference does, and the stand-alone kernel runs before the following iteration
            if (!pt_fresh) JRX_TRY(o.refresh_pt(cur));
            pt_fresh = !observed;
        }
        if (o.fusable && !observed) {
            JRX_TRY(o.fused(cur));
            h->stat_thermal_fused++;
            cur ^= 1;
        } else JRX_TRY(o.two_kernels(cur, observed, O::PH && pt_fresh));
        iter++;
        if (iter % p.nout == 0) {
            JRX_TRY(o.residual(cur));
            RedArr Z = {nullptr, {0, 0, 0}, 0}, A3 = {t.ResT, {o.n[0], o.n[1], o.n[2]}, 0};
            int nb = (int)((n + 2047) / 2048);
            nb = nb < 1 ? 1 : (nb > kMaxRedBlocks ? kMaxRedBlocks : nb);
            hipLaunchKernelGGL(k_sumsq_partial, dim3(nb), dim3(256), 0, s, Z, Z, Z, A3, h->d_partials);
            JRX_LAUNCH_CHECK(h);
            hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, s, h->d_partials, nb, h->d_sums);
            JRX_LAUNCH_CHECK(h);
            JRX_HIP(h, hipMemcpyAsync(h->h_sums, h->d_sums, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
            JRX_HIP(h, hipStreamSynchronize(s));
            err = sqrt(h->h_sums[3]) * sq;          // norm(ResT) * _sq_len_RT : local norm, no reduction across ranks (:131)
            // The reference stops each rank on its own local norm (no MPI reduction at :131); with an exchange in every iteration ranks that
            // cross ϵ at different checks would then wait for each other for ever.  Deviation: with more than one rank the loop test uses the
            // maximum of the local norms, so that all ranks leave together; the reported norm_ResT stays the local one.
            double err_stop = err;
            if (jrx_comm_active(h)) JRX_TRY(jrx_allreduce_host(h, &err_stop, 1, 1));
            if (cnt < cap) {
                if (norm_ResT) norm_ResT[cnt] = err;
                if (iter_count) iter_count[cnt] = iter;
            }
            cnt++;
            if (p.verbose && jrx_comm_rank(h) == 0) printf("iter = %lld, err = %1.3e \n", (long long)iter, err);
            err = err_stop;
        }
    }
    gexec.reset();      // here, not after the wait below: the runtime releases a graph that is still running once it has finished, and the host work of it hides behind the device's
    if (cur) JRX_TRY(o.copy_back());      // leave the results in the caller's arrays
    hipLaunchKernelGGL(k_sub, dim3(O::SUB_BLOCKS), dim3(256), 0, s, t.dT, (const double *)t.T, (const double *)t.Told, (i64)o.nodes());   // update_ΔT!
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(s));
    if (nnorms) *nnorms = cnt < cap ? cnt : cap;
    return JRX_OK;
}

}   // namespace
