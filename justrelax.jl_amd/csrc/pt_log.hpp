// pt_log.hpp -- the convergence log of the pseudo-transient Stokes drivers: err and its first value, the histories of jrx_solve_result, the reference's progress line
// and the result fields every exit fills.  Host only and free of HIP (tests/host/pt_log_harness.cpp builds it with g++ alone).  What differs between the drivers
// stays with them: the residual launches, the denominators of the norms, the loop rule and the condition for printing.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include "jrx.h"

class PtLog {
    jrx_solve_result *res;
    double err_, err_it1_ = 1.0;
    int64_t cont = 0;

    double put(int64_t iter, double e, double nRx, double nRy, const double *nRz, double nDV)
    {
        err_ = (std::isnan(nRx) || std::isnan(nRy) || (nRz && std::isnan(*nRz)) || std::isnan(nDV)) ? NAN : e;
        if (cont < res->cap) {
            if (res->norm_Rx) res->norm_Rx[cont] = nRx;
            if (res->norm_Ry) res->norm_Ry[cont] = nRy;
            if (nRz && res->norm_Rz) res->norm_Rz[cont] = *nRz;
            if (res->norm_divV) res->norm_divV[cont] = nDV;
            if (res->err_evo1) res->err_evo1[cont] = err_;
            if (res->err_evo2) res->err_evo2[cont] = iter;
        }
        if (cont == 0) err_it1_ = err_;
        cont++;
        return err_;
    }

public:
    // err0: err before the first check (INFINITY in the drivers whose reference starts there)
    explicit PtLog(jrx_solve_result *r, double err0 = 1.0) : res(r), err_(err0) {}
    double err() const { return err_; }
    double err_it1() const { return err_it1_; }
    double rel() const { return err_ / err_it1_; }

    // one check: err = the maximum of the norms, NaN if any of them is; the histories up to res->cap entries; returns err.  The 2D form leaves norm_Rz alone
    double record(int64_t iter, double nRx, double nRy, double nDV) { return put(iter, fmax(nRx, fmax(nRy, nDV)), nRx, nRy, nullptr, nDV); }
    double record(int64_t iter, double nRx, double nRy, double nRz, double nDV) { return put(iter, fmax(fmax(nRx, nRy), fmax(nRz, nDV)), nRx, nRy, &nRz, nDV); }

    void print2d(int64_t iter, double nRx, double nRy, double nDV) const
    {
        printf("Total steps = %lld, abs_err = %1.3e , rel_err = %1.3e [norm_Rx=%1.3e, norm_Ry=%1.3e, norm_∇V=%1.3e] \n",
               (long long)iter, err_, rel(), nRx, nRy, nDV);
    }
    void print3d(int64_t iter, double nRx, double nRy, double nRz, double nDV) const
    {
        printf("iter = %lld, abs_err = %1.3e, rel_err = %1.3e [norm_Rx=%1.3e, norm_Ry=%1.3e, norm_Rz=%1.3e, norm_∇V=%1.3e] \n",
               (long long)iter, err_, rel(), nRx, nRy, nRz, nDV);
    }

    // ms: the loop's elapsed time in milliseconds
    void finish(int64_t iter, double ms)
    {
        res->iter = iter;
        res->nchecks = cont < res->cap ? cont : res->cap;
        res->time_s = ms * 1e-3;
        res->av_time_s = iter > 1 ? res->time_s / (double)(iter - 1) : res->time_s;
    }
    // error("NaN(s)"); H: jrx_handle, or whatever jrx_fail is declared for (the header knows neither)
    template <class H>
    jrx_status fail_nan(H *h, int64_t iter, double ms)
    {
        finish(iter, ms);
        return jrx_fail(h, JRX_ERR_NAN, "NaN(s)");
    }
};
