// heat_plan_harness.cpp -- known answers for csrc/heat_plan.hpp (which iterations of the heat-diffusion PT loop are observed; the tile of the 3D one-launch kernels), built with
// g++ under -fsanitize=address,undefined (tests/test_host_heat_plan.py).  The cadence is walked as heat_solve (csrc/thermal_common.hpp) walks it: a run of unobserved
// iterations replays in whole graphs of 32, the rest as single launches; the counts are those of tests/_heat_diffusion.py (expected_fused, expected_replays).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "heat_plan.hpp"

using namespace heat_plan;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Walk { int64_t unobserved, graphs, singles, observed, last_observed; };
static Walk walk(int64_t iterMax, int64_t nout)
{
    Walk w = {0, 0, 0, 0, 0};
    int64_t iter = 0;
    while (iter < iterMax) {
        int64_t run = unobserved_run(iter, nout, iterMax);
        const int64_t nxt = next_observed(iter, nout, iterMax);
        CHECK(run >= 0 && nxt > iter && nxt <= iterMax && (nxt % nout == 0 || nxt == iterMax));
        // the three spellings agree, and with the plain one: the multiples of nout and the last iteration
        CHECK(observes_next(iter, nout, iterMax) == (run == 0));
        CHECK(observes_next(iter, nout, iterMax) == ((iter + 1) % nout == 0 || iter + 1 >= iterMax));
        if (run >= kGraphIters) {
            for (; run >= kGraphIters; run -= kGraphIters) { iter += kGraphIters; w.graphs++; w.unobserved += kGraphIters; }
            continue;
        }
        if (run == 0) { w.observed++; w.last_observed = iter + 1; }
        else { w.unobserved++; w.singles++; }
        iter++;
    }
    CHECK(iter == iterMax && w.last_observed == iterMax);
    CHECK(w.unobserved + w.observed == iterMax);
    return w;
}

static void cadence()
{
    CHECK(kGraphIters == 32);
    struct { int64_t iterMax, nout, unobserved, graphs, singles; } const known[] = {
        {45, 20, 42, 0, 42}, {70, 7, 60, 0, 60}, {99, 33, 96, 3, 0}, {300, 100, 297, 9, 9}, {102, 34, 99, 3, 3},
        {4000, 1000000000, 3999, 124, 31},      // the benchmark's cadence
        {1, 1, 0, 0, 0}, {1, 5, 0, 0, 0},       // iterMax = 1: the only iteration is observed
        {40, 1, 0, 0, 0},                       // nout = 1: every iteration is observed
        {10, 50, 9, 0, 9}, {33, 50, 32, 1, 0}, {34, 50, 33, 1, 1},      // nout > iterMax: only the last one
    };
    for (const auto &k : known) {
        const Walk w = walk(k.iterMax, k.nout);
        CHECK(w.unobserved == k.unobserved && w.graphs == k.graphs && w.singles == k.singles);
    }
    CHECK(walk(45, 20).observed == 3 && walk(40, 1).observed == 40 && walk(10, 50).observed == 1);
    CHECK(next_observed(0, 20, 45) == 20 && next_observed(19, 20, 45) == 20 && next_observed(20, 20, 45) == 40 && next_observed(40, 20, 45) == 45 && next_observed(44, 20, 45) == 45);
    for (int64_t iterMax = 1; iterMax <= 70; iterMax++)
        for (int64_t nout = 1; nout <= 72; nout++) walk(iterMax, nout);
}

static bool is(const Tile3 &t, int TX, int R, int KZ) { return t.TX == TX && t.R == R && t.KZ == KZ; }

static void tiles()
{
    // the default plan (cfg = 0, xg = 8): TX by nx, 4 planes, halved while the launch has fewer than 4096 waves
    struct { int nx, ny, nz, TX, KZ; } const known[] = {{16, 16, 16, 64, 1}, {48, 48, 48, 64, 1}, {64, 64, 64, 64, 1}, {96, 96, 96, 128, 4}, {256, 256, 256, 256, 4},
                                                          {130, 5, 9, 256, 1}, {65, 16, 6, 128, 1}, {128, 128, 128, 128, 4}, {129, 2, 2, 256, 1}, {64, 64, 127, 64, 2}};
    for (const auto &k : known) {
        const Tile3 t = tile3d(k.nx, k.ny, k.nz, 0, 8);
        CHECK(is(t, k.TX, 1, k.KZ));
        CHECK(t.ntx == (k.nx + k.TX - 1) / k.TX && t.nty == k.ny && t.ntz == (k.nz + k.KZ - 1) / k.KZ);
        CHECK(fused_shape_built(t, 8) && fused_ph_shape_built(t));
    }
    // 64 x 64 x 127: 64 rows of one wave in 32 chunks of 4 planes are 2048 waves, in 64 chunks of 2 planes 4096
    CHECK(tile3d(64, 64, 128, 0, 8).KZ == 2 && tile3d(64, 64, 126, 0, 8).KZ == 1);
    const Tile3 a = tile3d(130, 5, 9, 0, 8);
    CHECK(a.ntx == 1 && a.nty == 5 && a.ntz == 9);
    // "thermal_cfg" = R*10000 + (TX/64)*100 + KZ is taken as it is, on small grids too
    CHECK(is(tile3d(20, 9, 7, 10104, 8), 64, 1, 4) && is(tile3d(20, 9, 7, 20404, 8), 256, 2, 4) && is(tile3d(130, 5, 9, 10408, 8), 256, 1, 8));
    const Tile3 b = tile3d(20, 9, 7, 20404, 8);
    CHECK(b.ntx == 1 && b.nty == 5 && b.ntz == 2);
    const Tile3 c = tile3d(130, 5, 9, 10408, 8);
    CHECK(c.ntx == 1 && c.nty == 5 && c.ntz == 2);
    for (int cfg : {10104, 20404, 10408, 10102, 10204, 10202, 10404, 10402}) CHECK(fused_shape_built(tile3d(130, 5, 9, cfg, 8), 8));
    CHECK(!fused_shape_built(tile3d(130, 5, 9, 30404, 8), 8) && !fused_ph_shape_built(tile3d(130, 5, 9, 20404, 8)) && !fused_ph_shape_built(tile3d(130, 5, 9, 10408, 8)));
    // the shallower chunks exist for the default XCD band width only: with "thermal_xg" != 8 the depth stays 4
    for (int xg : {1, 2, 4}) {
        CHECK(is(tile3d(16, 16, 16, 0, xg), 64, 1, 4) && is(tile3d(130, 5, 9, 0, xg), 256, 1, 4));
        CHECK(fused_shape_built(tile3d(256, 256, 256, 0, xg), xg));
    }
    // every shape the default plan can return is one the dispatch instantiates, in both forms
    for (int TX : {64, 128, 256})
        for (int KZ : {1, 2, 4}) {
            const Tile3 t = {TX, 1, KZ, 1, 1, 1};
            CHECK(fused_shape_built(t, 8) && fused_ph_shape_built(t));
        }
    for (int nx = 2; nx <= 300; nx += 7)
        for (int ny = 2; ny <= 300; ny += 23)
            for (int nz = 2; nz <= 300; nz += 19) {
                const Tile3 t = tile3d(nx, ny, nz, 0, 8);
                CHECK((t.TX == 64 || t.TX == 128 || t.TX == 256) && (t.KZ == 1 || t.KZ == 2 || t.KZ == 4) && t.R == 1);
                CHECK(t.TX >= nx || t.TX == 256);
                CHECK(t.KZ == 4 || (int64_t)t.ntx * (t.TX / 64) * ny * ((nz + 2 * t.KZ - 1) / (2 * t.KZ)) < 4096);      // a depth was halved only below 4096 waves
                CHECK(t.KZ == 1 || (int64_t)t.ntx * (t.TX / 64) * ny * t.ntz >= 4096);                                  // ... and halving stopped at 4096
            }
}

int main()
{
    cadence();
    tiles();
    printf("ok\n");
    return 0;
}
