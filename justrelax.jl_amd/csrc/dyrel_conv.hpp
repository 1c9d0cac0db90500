// dyrel_conv.hpp -- the convergence bookkeeping of the DYREL solve loop (dyrel_common.hpp), for ND = 2 or 3 velocity components: everything between "the sums are on
// the host" and "what the loop does next".  Host only and free of HIP (tests/host/dyrel_conv_harness.cpp builds it with g++ alone).
//
// Reference (PTsolvers/JustRelax.jl): src/DYREL/solver.jl:151-183 (the Powell-Hestenes norms, err, the exits, rel_drop), :231-252 (the residual check of the inner
// loop, the histories, cV), :349-365 (velocity_dofs, pressure_dof, compute_λminV!).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include "jrx.h"

enum DyVerdict { DY_CONTINUE, DY_CONVERGED, DY_NAN, DY_KABOOM };

template <int ND>
class DyrelConv {
    static_assert(ND == 2 || ND == 3, "2D or 3D");
    static constexpr double EPS = 2.220446049250313e-16;
    const jrx_dyrel2d_params *dp;
    jrx_dyrel2d_result *res;
    double dofs[ND], pdof;      // velocity_dofs, pressure_dof
    double err_, err_min = INFINITY, errV0[ND], errPt0 = 1.0, errV00 = 1.0, errPt = 1.0, rel_drop, eps_vel_ = 0.0;
    int64_t cont = 0;

public:
    DyrelConv(const jrx_dyrel2d_params *dp_, jrx_dyrel2d_result *r, const double dofs_[ND], double pdof_) : dp(dp_), res(r), pdof(pdof_), err_(2 * dp_->eps), rel_drop(dp_->rel_drop)
    {
        for (int c = 0; c < ND; c++) { dofs[c] = dofs_[c]; errV0[c] = 1.0; }
    }
    double err() const { return err_; }
    double eps_vel() const { return eps_vel_; }      // err * rel_drop of the last outer step that went on

    // one Powell-Hestenes iteration: S = Σ R_c² (ND of them), Σ RP².  nx: the divisor of the progress line
    DyVerdict outer(int64_t itPH, int64_t iter, int64_t nx, const double *S)
    {
        double errV[ND];
        for (int c = 0; c < ND; c++) errV[c] = sqrt(S[c]) / sqrt(dofs[c]);
        errPt = sqrt(S[ND]) / sqrt(pdof);
        if (itPH == 1) { for (int c = 0; c < ND; c++) errV0[c] = errV[c] + EPS; errPt0 = errPt + EPS; }
        if (itPH == 2) errPt0 = errPt + EPS;
        err_ = fmin(errPt / errPt0, errPt);
        bool nan = std::isnan(err_);
        for (int c = 0; c < ND; c++) {
            const double e = fmin(errV[c] / errV0[c], errV[c]);
            err_ = fmax(err_, e);
            nan = nan || std::isnan(e);      // fmax alone would drop a NaN
        }
        if (nan) err_ = NAN;
        if (dp->verbose_PH) {
            if constexpr (ND == 2)
                printf("itPH = %02lld iter = %06lld iter/nx = %03lld, err = %1.3e - norm[R1=%1.3e %1.3e, R2=%1.3e %1.3e, Rp=%1.3e %1.3e] \n", (long long)itPH, (long long)iter,
                       (long long)(iter / nx), err_, errV[0], errV[0] / errV0[0], errV[1], errV[1] / errV0[1], errPt, errPt / errPt0);
            else
                printf("itPH = %02lld iter = %06lld iter/nx = %03lld, err = %1.3e - norm[R1=%1.3e %1.3e, R2=%1.3e %1.3e, R3=%1.3e %1.3e, Rp=%1.3e %1.3e] \n", (long long)itPH,
                       (long long)iter, (long long)(iter / nx), err_, errV[0], errV[0] / errV0[0], errV[1], errV[1] / errV0[1], errV[2], errV[2] / errV0[2], errPt, errPt / errPt0);
        }
        if (std::isnan(err_)) return DY_NAN;
        if (err_ > 1.0e10) return DY_KABOOM;
        if (err_ < dp->eps) return DY_CONVERGED;
        if (err_ > err_min * 1.05) rel_drop = fmax(rel_drop * 0.1, 1.0e-3);
        if (err_min > err_) err_min = err_;
        eps_vel_ = err_ * rel_drop;
        return DY_CONTINUE;
    }

    // one residual check of the inner loop: S = Σ (D R)_c², Σ dV_c (R - R0)_c, Σ dV_c² (ND of each).  Leaves cV of update_cV! in *cV; false: NaN, the loop ends
    bool inner(int64_t itPT, int64_t iter, const double *S, double *cV)
    {
        double eV[ND], emax = 0.0;
        bool nan = false;
        for (int c = 0; c < ND; c++) {
            eV[c] = sqrt(S[c]) / sqrt(dofs[c]);
            emax = c ? fmax(emax, eV[c]) : eV[c];
            nan = nan || std::isnan(eV[c]);
        }
        if (iter == dp->nout) errV00 = emax + EPS;
        err_ = eV[0] / errV00;
        for (int c = 1; c < ND; c++) err_ = fmax(err_, eV[c] / errV00);
        if (nan) err_ = NAN;
        if (cont < res->cap) {
            if (res->err_evo_tot) res->err_evo_tot[cont] = err_;
            if (res->err_evo_V) res->err_evo_V[cont] = err_;
            if (res->err_evo_P) res->err_evo_P[cont] = errPt / errPt0;
            if (res->err_evo_it) res->err_evo_it[cont] = (double)iter;
        }
        cont++;
        if (std::isnan(err_)) return false;
        if (dp->verbose_DR) printf("it = %lld, iter = %lld, err = %1.3e \n", (long long)itPT, (long long)iter, err_);
        double num = S[ND], den = S[2 * ND];      // compute_λminV! :359-365, each sum left to right
        for (int c = 1; c < ND; c++) { num += S[ND + c]; den += S[2 * ND + c]; }
        *cV = 2 * sqrt(fabs(num) / den) * dp->c_fact;
        return true;
    }

    // ms: the loop's elapsed time in milliseconds
    void finish(int64_t iter, int64_t itPH, double ms)
    {
        res->iter = iter; res->itPH = itPH;
        res->nchecks = cont < res->cap ? cont : res->cap;
        res->time_s = ms * 1e-3;
    }
};
