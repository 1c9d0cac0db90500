// dyrel_conv_harness.cpp -- known answers for csrc/dyrel_conv.hpp (the convergence bookkeeping of the DYREL solve loop, ND = 2 and 3), built with g++ under
// -fsanitize=address,undefined (tests/test_host_dyrel_conv.py).  The inputs are powers of two, so every expected value below is exact and worked by hand.
// The history arrays are heap blocks of exactly `cap` entries: a write past the cap guard is an AddressSanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dyrel_conv.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static const double KEEP = -77.25;      // what an untouched entry holds
static const double E = 2.220446049250313e-16, P2_53 = E / 2, TINY = 1.0 / 1024;      // 2^-52, 2^-53, 2^-10

static jrx_dyrel2d_params params(double eps = 1.0 / (1 << 30))
{
    jrx_dyrel2d_params dp;
    memset(&dp, 0, sizeof(dp));
    dp.eps = eps; dp.rel_drop = 0.5; dp.nout = 10; dp.c_fact = 0.5;
    return dp;
}

struct Hist {
    std::vector<double> it, V, P, tot;
    jrx_dyrel2d_result res;
    // skip: which of the four arrays is NULL (-1: none)
    Hist(int cap, int slots, int skip = -1) : it(slots, KEEP), V(slots, KEEP), P(slots, KEEP), tot(slots, KEEP)
    {
        memset(&res, 0, sizeof(res));
        res.cap = cap;
        res.iter = res.itPH = res.nchecks = -1; res.time_s = -1.0;
        res.err_evo_it = skip == 0 ? nullptr : it.data(); res.err_evo_V = skip == 1 ? nullptr : V.data();
        res.err_evo_P = skip == 2 ? nullptr : P.data(); res.err_evo_tot = skip == 3 ? nullptr : tot.data();
    }
};

// dofs 4, 16[, 64] and 4^(ND+1) pressure dofs: the norm of component c is sqrt(S[c]) / 2^(c+1)
template <int ND>
struct Case {
    jrx_dyrel2d_params dp;
    Hist hst;
    DyrelConv<ND> conv;
    static constexpr double dofs[3] = {4.0, 16.0, 64.0};
    Case(const jrx_dyrel2d_params &dp_, int cap = 4, int slots = 4, int skip = -1) : dp(dp_), hst(cap, slots, skip), conv(&dp, &hst.res, dofs, ND == 2 ? 64.0 : 256.0) {}
    // the outer step whose norms are n[0..ND-1] (velocity) and n[ND] (pressure)
    DyVerdict outer(int64_t itPH, const double *n, int64_t iter = 0)
    {
        double S[ND + 1];
        for (int c = 0; c <= ND; c++) { const double r = n[c] * (double)(2 << c); S[c] = r * r; }
        return conv.outer(itPH, iter, 100, S);
    }
    // the outer step with the velocity norm v in component `at`, TINY / 4 elsewhere: err = v by the abs branch once the references are TINY-sized
    DyVerdict outer1(int64_t itPH, double v, int at = 0)
    {
        double n[ND + 1];
        for (int c = 0; c <= ND; c++) n[c] = c == at ? v : TINY / 4;
        return outer(itPH, n);
    }
};

template <int ND>
static void references_and_branches()
{
    Case<ND> k(params());
    double a1[ND + 1] = {2.0, 2.0, 2.0}, a2[ND + 1] = {4.0, 1.0, 1.0}, a3[ND + 1] = {8.0, 1.0, 1.0};
    a1[ND] = 4.0; a2[ND] = 2.0; a3[ND] = 4.0;      // the pressure norms
    CHECK(k.conv.err() == 2 * k.dp.eps);
    // itPH 1: the references are the norms themselves (2 + eps = 2): rel = 1 < abs
    CHECK(k.outer(1, a1) == DY_CONTINUE && k.conv.err() == 1.0 && k.conv.eps_vel() == 0.5);
    // itPH 2: errV0 stays (4 / 2 = 2 < 4, rel; 1 / 2 < 1, rel), errPt0 is taken again (2 / 2 = 1, not 2 / 4)
    CHECK(k.outer(2, a2) == DY_CONTINUE && k.conv.err() == 2.0);
    // itPH 3: neither is taken again: 8 / 2 = 4 in the velocity (2 with a reference of itPH 2), 4 / 2 = 2 in the pressure (1 with the reference of itPH 1 or 3)
    CHECK(k.outer(3, a3) == DY_CONTINUE && k.conv.err() == 4.0);
    double S[9] = {64.0, 64.0, 64.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, cV;
    CHECK(k.conv.inner(1, 30, S, &cV) && k.hst.P[0] == 2.0);      // err_evo_P = errPt / errPt0

    // below one the abs branch wins and "+ eps" shows: 0.5 / (0.5 + eps) < 1 but > 0.5
    Case<ND> lo(params());
    const double h[4] = {0.5, 0.5, 0.5, 0.5};
    CHECK(lo.outer(1, h) == DY_CONTINUE && lo.conv.err() == 0.5);
    const double q[4] = {0.25, 0.25, 0.25, 0.25};      // 0.25 / (0.5 + eps) > 0.25: abs; errPt0 again: 0.25 / (0.25 + eps) > 0.25: abs
    CHECK(lo.outer(2, q) == DY_CONTINUE && lo.conv.err() == 0.25);
    // each velocity component alone decides the maximum
    for (int at = 0; at < ND; at++) {
        Case<ND> m(params());
        CHECK(m.outer(1, h) == DY_CONTINUE);
        double w[ND + 1];
        for (int c = 0; c <= ND; c++) w[c] = c == at ? 1.0 : 0.25;
        CHECK(m.outer(2, w) == DY_CONTINUE && m.conv.err() == 1.0);      // min(1 / (0.5 + eps), 1) = 1
    }
    // all-zero residuals: 0 / (0 + eps) = 0, converged and not 0 / 0
    Case<ND> z(params());
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    CHECK(z.outer(1, zero) == DY_CONVERGED && z.conv.err() == 0.0);
}

template <int ND>
static void verdicts()
{
    const double big = 1099511627776.0;      // 2^40 > 1e10
    for (int at = 0; at <= ND; at++) {
        Case<ND> k(params());
        CHECK(k.outer1(1, TINY) == DY_CONTINUE);
        double n[ND + 1];
        for (int c = 0; c <= ND; c++) n[c] = big;
        CHECK(k.outer(2, n) == DY_KABOOM && k.conv.err() == big);
        n[at] = NAN;      // NaN goes first, whatever the others are
        CHECK(k.outer(3, n) == DY_NAN && std::isnan(k.conv.err()));
    }
    CHECK(fmax(NAN, 1.0) == 1.0);      // fmax alone would drop a NaN: the rule is explicit
    Case<ND> r(params());
    CHECK(r.outer1(1, 1.0) == DY_CONTINUE && r.conv.err() == 1.0 - E);      // the rel branch shows "+ eps": 1 / (1 + 2^-52) = 1 - 2^-52 < 1
    Case<ND> c(params(TINY / 2));
    CHECK(c.outer1(1, TINY) == DY_CONTINUE && c.conv.err() == TINY);      // not < eps
    CHECK(c.outer1(2, TINY / 4) == DY_CONVERGED && c.conv.err() == TINY / 4);
}

template <int ND>
static void rel_drop_rule()
{
    // rising err: 0.5 -> 0.05 -> 0.005 -> 0.001 and it holds there
    Case<ND> k(params());
    CHECK(k.outer1(1, TINY) == DY_CONTINUE && k.conv.err() == TINY && k.conv.eps_vel() == TINY * 0.5);      // err_min was Inf: no drop
    const double r1 = 0.5 * 0.1, r2 = r1 * 0.1;
    CHECK(r2 * 0.1 < 1.0e-3);
    CHECK(k.outer1(2, 0.25) == DY_CONTINUE && k.conv.eps_vel() == 0.25 * r1);
    CHECK(k.outer1(3, 0.5) == DY_CONTINUE && k.conv.eps_vel() == 0.5 * r2);
    CHECK(k.outer1(4, 1.0) == DY_CONTINUE && k.conv.eps_vel() == 1.0 * 1.0e-3);
    CHECK(k.outer1(5, 2.0) == DY_CONTINUE && k.conv.eps_vel() == 2.0 * 1.0e-3);
    // the 5 % band, and err_min lowered only after the comparison: 1, 0.5 (new minimum: no drop), 0.5 * 1.03125 (inside the band of 0.5), 0.5 * 1.0625 (outside it;
    // inside the band of 1, so a minimum that had stayed at 1 would not drop)
    Case<ND> b(params());
    CHECK(b.outer1(1, TINY) == DY_CONTINUE && b.conv.eps_vel() == TINY * 0.5);
    CHECK(b.outer1(2, TINY * 0.5) == DY_CONTINUE && b.conv.eps_vel() == TINY * 0.5 * 0.5);
    CHECK(b.outer1(3, TINY * 0.5 * 1.03125) == DY_CONTINUE && b.conv.eps_vel() == TINY * 0.5 * 1.03125 * 0.5);
    CHECK(b.outer1(4, TINY * 0.5 * 1.0625) == DY_CONTINUE && b.conv.eps_vel() == TINY * 0.5 * 1.0625 * r1);
    // a comparison against the minimum already lowered by the same err could never fire on a falling err; neither does this one
    CHECK(b.outer1(5, TINY * 0.25) == DY_CONTINUE && b.conv.eps_vel() == TINY * 0.25 * r1);
}

template <int ND>
static void inner_checks()
{
    // eV = sqrt(S[c]) / 2^(c+1); errV00 only when iter == nout (10)
    Case<ND> k(params(), 2, 2);      // two entries allocated: a third write is out of bounds
    double S[9] = {64.0, 64.0, 64.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cV = KEEP;      // eV = 4, 2[, 1]
    S[ND] = -4.0; S[2 * ND] = 1.0;      // λmin = |-4| / 1, cV = 2 sqrt(4) c_fact = 2
    CHECK(k.conv.inner(3, 10, S, &cV) && k.conv.err() == 1.0 && cV == 2.0);      // errV00 = 4 (+ eps = 4): 4 / 4
    S[0] = 16.0; S[1] = 1024.0;      // eV = 2, 8[, 1]
    S[ND] = 1.0; S[2 * ND] = 16.0;      // λmin = 1 / 16, cV = 2 (1 / 4) c_fact
    CHECK(k.conv.inner(3, 20, S, &cV) && k.conv.err() == 2.0 && cV == 0.25);      // 8 / 4: errV00 is not taken again
    CHECK(k.conv.inner(3, 30, S, &cV) && k.conv.err() == 2.0);      // counted, not written
    CHECK(k.hst.tot[0] == 1.0 && k.hst.V[0] == 1.0 && k.hst.it[0] == 10.0 && k.hst.P[0] == 1.0);      // errPt / errPt0 = 1 / 1 before any outer step
    CHECK(k.hst.tot[1] == 2.0 && k.hst.V[1] == 2.0 && k.hst.it[1] == 20.0 && k.hst.P[1] == 1.0);
    k.conv.finish(30, 4, 250.0f);
    CHECK(k.hst.res.nchecks == 2 && k.hst.res.iter == 30 && k.hst.res.itPH == 4 && k.hst.res.time_s == 250.0 * 1e-3);
    // a first check at another iteration leaves errV00 = 1; below the cap nchecks is the count and the entries behind stay
    Case<ND> l(params(), 3, 4);
    CHECK(l.conv.inner(1, 20, S, &cV) && l.conv.err() == 8.0);
    l.conv.finish(20, 1, 2.0);
    CHECK(l.hst.res.nchecks == 1 && l.hst.tot[1] == KEEP && l.hst.it[3] == KEEP);
    // cap = 0: nothing is written
    Case<ND> none(params(), 0, 1);
    CHECK(none.conv.inner(1, 10, S, &cV));
    none.conv.finish(10, 1, 1.0);
    CHECK(none.hst.res.nchecks == 0 && none.hst.tot[0] == KEEP && none.hst.it[0] == KEEP);
    // each history NULL in turn
    for (int skip = 0; skip < 4; skip++) {
        Case<ND> n(params(), 2, 2, skip);
        CHECK(n.conv.inner(1, 10, S, &cV) && n.conv.inner(1, 20, S, &cV));
        const double got[4] = {n.hst.it[1], n.hst.V[1], n.hst.P[1], n.hst.tot[1]}, want[4] = {20.0, 1.0, 1.0, 1.0};      // errV00 = 8: 8 / 8
        for (int a = 0; a < 4; a++) CHECK(got[a] == (a == skip ? KEEP : want[a]));
    }
    // NaN in each position: recorded, counted, the loop ends, cV is left alone
    for (int at = 0; at < ND; at++) {
        Case<ND> n(params(), 2, 2);
        double T[9] = {64.0, 64.0, 64.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
        T[at] = NAN;
        cV = KEEP;
        CHECK(!n.conv.inner(1, 10, T, &cV) && std::isnan(n.conv.err()) && cV == KEEP);
        CHECK(std::isnan(n.hst.tot[0]) && std::isnan(n.hst.V[0]) && n.hst.it[0] == 10.0);
        n.conv.finish(10, 1, 1.0);
        CHECK(n.hst.res.nchecks == 1);
    }
}

// compute_λminV!: each sum left to right.  (1 + 2^-53) + -1 = 0 where 1 + (2^-53 + -1) = 2^-53; (1 + 2^-53) + 2^-53 = 1 where 1 + (2^-53 + 2^-53) = 1 + 2^-52,
// and 2 sqrt(4 / (1 + 2^-52)) c_fact = 2 - 2^-52, the double below 2
static void lambda_min_association()
{
    Case<3> k(params());
    double cV = KEEP;
    const double num[9] = {64.0, 64.0, 64.0, 1.0, P2_53, -1.0, 1.0, 0.0, 0.0};
    CHECK(k.conv.inner(1, 10, num, &cV) && cV == 0.0);
    const double den[9] = {64.0, 64.0, 64.0, 4.0, 0.0, 0.0, 1.0, P2_53, P2_53};
    CHECK(1.0 + (P2_53 + P2_53) == 1.0 + E && 2 * sqrt(4.0 / (1.0 + E)) * 0.5 == 2.0 - E);
    CHECK(k.conv.inner(1, 20, den, &cV) && cV == 2.0);
}

template <int ND>
static void print_lines()
{
    jrx_dyrel2d_params dp = params();
    dp.verbose_PH = dp.verbose_DR = 1; dp.nout = 100;
    Case<ND> k(dp);
    const double a1[4] = {2.0, 2.0, ND == 2 ? 4.0 : 2.0, 4.0}, a2[4] = {4.0, 1.0, ND == 2 ? 2.0 : 4.0, 2.0};
    k.outer(1, a1, 0);
    k.outer(2, a2, 1234);
    double S[9] = {64.0, 64.0, 64.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, cV;
    k.conv.inner(34, 1300, S, &cV);
}

template <int ND>
static void all()
{
    references_and_branches<ND>();
    verdicts<ND>();
    rel_drop_rule<ND>();
    inner_checks<ND>();
    print_lines<ND>();
}

int main()
{
    all<2>();
    all<3>();
    lambda_min_association();
    printf("ok\n");
    return 0;
}
