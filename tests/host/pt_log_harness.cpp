// pt_log_harness.cpp -- known answers for csrc/pt_log.hpp (the convergence log of the PT Stokes drivers), built with g++ under -fsanitize=address,undefined
// (tests/test_host_pt_log.py).  The history arrays are heap blocks of exactly `cap` entries plus nothing: a write past the cap guard is an AddressSanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pt_log.hpp"

struct FakeHandle { char err[64]; };
static jrx_status jrx_fail(FakeHandle *h, jrx_status st, const char *msg)
{
    snprintf(h->err, sizeof(h->err), "%s", msg);
    return st;
}

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static const double KEEP = -77.25;      // what an untouched entry holds

struct Hist {
    std::vector<double> e1, rx, ry, rz, dv;
    std::vector<int64_t> e2;
    jrx_solve_result res;
    // skip: which of the six arrays is NULL (-1: none)
    Hist(int cap, int slots, int skip = -1) : e1(slots, KEEP), rx(slots, KEEP), ry(slots, KEEP), rz(slots, KEEP), dv(slots, KEEP), e2(slots, -7)
    {
        memset(&res, 0, sizeof(res));
        res.cap = cap;
        res.iter = res.nchecks = -1; res.time_s = res.av_time_s = -1.0;
        res.err_evo1 = skip == 0 ? nullptr : e1.data(); res.err_evo2 = skip == 1 ? nullptr : e2.data();
        res.norm_Rx = skip == 2 ? nullptr : rx.data(); res.norm_Ry = skip == 3 ? nullptr : ry.data();
        res.norm_Rz = skip == 4 ? nullptr : rz.data(); res.norm_divV = skip == 5 ? nullptr : dv.data();
    }
};

static void cap_guard()
{
    Hist hst(2, 2);      // two entries allocated: a third write is out of bounds
    PtLog log(&hst.res);
    CHECK(log.err() == 1.0 && log.err_it1() == 1.0 && log.rel() == 1.0);
    CHECK(log.record(10, 4.0, 2.0, 3.0, 1.0) == 4.0);
    CHECK(log.record(20, 0.5, 2.0, 1.0, 0.25) == 2.0);
    CHECK(log.record(30, 0.5, 0.125, 1.0, 0.25) == 1.0);
    CHECK(hst.e1[0] == 4.0 && hst.e1[1] == 2.0 && hst.e2[0] == 10 && hst.e2[1] == 20);
    CHECK(hst.rx[0] == 4.0 && hst.rx[1] == 0.5 && hst.ry[0] == 2.0 && hst.ry[1] == 2.0 && hst.rz[0] == 3.0 && hst.rz[1] == 1.0 && hst.dv[0] == 1.0 && hst.dv[1] == 0.25);
    CHECK(log.err() == 1.0 && log.err_it1() == 4.0 && log.rel() == 0.25);      // err_it1 from the first call only; err follows the third, unrecorded one
    log.finish(30, 500.0);
    CHECK(hst.res.nchecks == 2 && hst.res.iter == 30);
    // with room to spare the entries behind the recorded ones stay as they were
    Hist big(2, 4);
    PtLog lb(&big.res);
    for (int q = 0; q < 3; q++) lb.record(q + 1, 1.0, 2.0, 3.0, 4.0);
    for (int q = 2; q < 4; q++)
        CHECK(big.e1[q] == KEEP && big.e2[q] == -7 && big.rx[q] == KEEP && big.ry[q] == KEEP && big.rz[q] == KEEP && big.dv[q] == KEEP);
    CHECK(big.e1[1] == 4.0 && big.e2[1] == 2);
    // cap = 0: nothing is written at all
    Hist none(0, 1);
    PtLog ln(&none.res);
    CHECK(ln.record(5, 1.0, 2.0, 3.0, 4.0) == 4.0);
    ln.finish(5, 1.0);
    CHECK(none.e1[0] == KEEP && none.e2[0] == -7 && none.res.nchecks == 0);
}

static void null_arrays()
{
    for (int skip = 0; skip < 6; skip++) {
        Hist hst(2, 2, skip);
        PtLog log(&hst.res);
        CHECK(log.record(3, 1.0, 2.0, 3.0, 4.0) == 4.0);
        CHECK(log.record(6, 8.0, 7.0, 6.0, 5.0) == 8.0);
        const double want[6][2] = {{4.0, 8.0}, {3.0, 6.0}, {1.0, 8.0}, {2.0, 7.0}, {3.0, 6.0}, {4.0, 5.0}};
        for (int q = 0; q < 2; q++) {
            const double got[6] = {hst.e1[q], (double)hst.e2[q], hst.rx[q], hst.ry[q], hst.rz[q], hst.dv[q]};
            for (int a = 0; a < 6; a++) CHECK(got[a] == (a == skip ? (a == 1 ? -7.0 : KEEP) : want[a][q]));
        }
    }
}

static void nan_rule()
{
    for (int which = 0; which < 4; which++) {
        double v[4] = {1.0, 2.0, 3.0, 4.0};
        v[which] = NAN;
        Hist hst(2, 2);
        PtLog log(&hst.res);
        CHECK(std::isnan(log.record(7, v[0], v[1], v[2], v[3])));
        CHECK(std::isnan(log.err()) && std::isnan(log.err_it1()) && std::isnan(hst.e1[0]) && hst.e2[0] == 7);
        CHECK(std::isnan(hst.rx[0]) == (which == 0) && std::isnan(hst.ry[0]) == (which == 1) && std::isnan(hst.rz[0]) == (which == 2) && std::isnan(hst.dv[0]) == (which == 3));
        if (which == 2) continue;
        double w[3] = {v[0], v[1], v[3]};
        Hist h2(2, 2);
        PtLog l2(&h2.res);
        CHECK(std::isnan(l2.record(7, w[0], w[1], w[2])) && std::isnan(h2.e1[0]));
    }
    // fmax alone would drop a NaN: the rule is explicit
    CHECK(fmax(NAN, 1.0) == 1.0);
}

static void form_2d()
{
    Hist hst(2, 2);
    PtLog log(&hst.res);
    CHECK(log.record(4, 1.0, 3.0, 2.0) == 3.0);
    CHECK(log.record(8, 0.5, 0.25, 2.0) == 2.0);
    CHECK(hst.rz[0] == KEEP && hst.rz[1] == KEEP);
    CHECK(hst.rx[0] == 1.0 && hst.ry[0] == 3.0 && hst.dv[0] == 2.0 && hst.e1[1] == 2.0 && hst.e2[1] == 8);
    CHECK(log.err_it1() == 3.0);
}

static void start_value()
{
    jrx_solve_result r;
    memset(&r, 0, sizeof(r));
    PtLog log(&r, INFINITY);
    CHECK(std::isinf(log.err()) && log.err_it1() == 1.0 && std::isinf(log.rel()));
}

static void times()
{
    for (int64_t iter = 0; iter < 3; iter++) {
        Hist hst(2, 2);
        PtLog log(&hst.res);
        log.finish(iter, 3000.0);
        const double t = 3000.0 * 1e-3;
        CHECK(hst.res.iter == iter && hst.res.nchecks == 0 && hst.res.time_s == t);
        CHECK(hst.res.av_time_s == (iter > 1 ? t / (double)(iter - 1) : t));
    }
    Hist hst(4, 4);
    PtLog log(&hst.res);
    log.record(5, 1.0, NAN, 1.0, 1.0);
    FakeHandle fh;
    fh.err[0] = 0;
    CHECK(log.fail_nan(&fh, 5, 250.0f) == JRX_ERR_NAN);
    CHECK(strcmp(fh.err, "NaN(s)") == 0);
    CHECK(hst.res.iter == 5 && hst.res.nchecks == 1 && hst.res.time_s == 250.0 * 1e-3 && hst.res.av_time_s == 250.0 * 1e-3 / 4.0);
}

static void print_lines()
{
    Hist hst(2, 2);
    PtLog log(&hst.res);
    log.record(1, 4.0, 2.0, 1.0, 0.5);
    log.record(2, 2.0, 1.0, 0.5, 0.25);
    log.print3d(2, 2.0, 1.0, 0.5, 0.25);
    log.print2d(2, 2.0, 1.0, 0.25);
}

int main()
{
    cap_guard();
    null_arrays();
    nan_rule();
    form_2d();
    start_value();
    times();
    print_lines();
    printf("ok\n");
    return 0;
}
