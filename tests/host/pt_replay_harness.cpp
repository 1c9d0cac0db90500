// pt_replay_harness.cpp -- known answers for csrc/pt_replay.hpp (which iterations of a PT loop are observed, and the run of unobserved ones a replay may take), built with
// g++ under -fsanitize=address,undefined (tests/test_host_pt_replay.py).  `last` is the last iteration a loop can run: iterMax + 1 for the Stokes loops, iterMax for the heat
// loop, whose forwards (csrc/heat_plan.hpp) must give what they gave before they were forwards (the cadence table of tests/host/heat_plan_harness.cpp).
#include <cstdio>
#include <cstdlib>
#include "pt_replay.hpp"
#include "heat_plan.hpp"

using namespace pt_replay;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// the window as the five Stokes loops spelled it by hand
static int64_t by_hand(int64_t iter, int64_t nout, int64_t iterMax, int64_t hold_back)
{
    int64_t nxt = ((iter / nout) + 1) * nout;
    if (nxt > iterMax + 1) nxt = iterMax + 1;
    return nxt - 1 - hold_back - iter;
}

// a Stokes loop (iter <= iterMax) walked as the drivers walk it from iteration `from` on: whole graphs of git while the run allows, single iterations otherwise
struct Walk { int64_t replays, singles, observed; };
static Walk walk(int64_t iterMax, int64_t nout, int git, int64_t hold_back, int64_t from)
{
    Walk w = {0, 0, 0};
    int64_t iter = 0;
    while (iter <= iterMax) {
        int64_t run = iter >= from ? unobserved_run(iter, nout, iterMax + 1, hold_back) : 0;
        if (run >= git) {
            for (; run >= git; run -= git) { iter += git; w.replays++; }
            continue;
        }
        if (observes_next(iter, nout, iterMax + 1)) w.observed++;
        else w.singles++;
        iter++;
    }
    CHECK(iter == iterMax + 1);
    return w;
}

static void stokes_windows()
{
    // the 2D VEP loop of tests/test_gpu_vep_extras.py: iterMax = 299, nout = 150
    CHECK(unobserved_run(1, 150, 300) == 148);
    CHECK(unobserved_run(150, 150, 300) == 149);
    CHECK(next_observed(1, 150, 300) == 150 && next_observed(149, 150, 300) == 150 && next_observed(150, 150, 300) == 300 && next_observed(299, 150, 300) == 300);
    // the SolCx loop of tests/test_gpu_stokes2d_thermal.py: iterMax = 399, nout = 200, one iteration held back
    CHECK(unobserved_run(2, 200, 400, 1) == 196);
    CHECK(unobserved_run(2, 200, 400) == 197 && unobserved_run(200, 200, 400, 1) == 198);
    // `last` inside the current window: it, not the next multiple of nout, is the next observed iteration
    CHECK(next_observed(100, 150, 130) == 130 && unobserved_run(100, 150, 130) == 29 && unobserved_run(100, 150, 130, 1) == 28);
    CHECK(next_observed(0, 1000, 24) == 24 && unobserved_run(0, 1000, 24) == 23);
    CHECK(next_observed(300, 100, 350) == 350 && unobserved_run(317, 100, 350) == 32);
    // `last` on a multiple of nout, and one past it
    CHECK(next_observed(250, 100, 300) == 300 && next_observed(250, 100, 301) == 300 && next_observed(300, 100, 301) == 301 && unobserved_run(300, 100, 301) == 0);
    // nout = 1: every iteration is observed, the run is never positive
    for (int64_t iter = 0; iter < 50; iter++) {
        CHECK(next_observed(iter, 1, 50) == iter + 1 && observes_next(iter, 1, 50));
        CHECK(unobserved_run(iter, 1, 50) == 0 && unobserved_run(iter, 1, 50, 1) == -1);
    }
    // one short of an observed iteration: nothing unobserved is left, and a hold-back makes the run negative, never a wrap-around
    CHECK(unobserved_run(149, 150, 300) == 0 && observes_next(149, 150, 300) && unobserved_run(149, 150, 300, 1) == -1);
    CHECK(unobserved_run(299, 150, 300) == 0 && observes_next(299, 150, 300));
    CHECK(unobserved_run(148, 150, 300) == 1 && !observes_next(148, 150, 300) && unobserved_run(148, 150, 300, 1) == 0);
    // against the hand-written window of the drivers, and the three spellings against one another
    for (int64_t iterMax = 1; iterMax <= 70; iterMax++)
        for (int64_t nout = 1; nout <= 72; nout++)
            for (int64_t iter = 0; iter <= iterMax; iter++) {
                const int64_t last = iterMax + 1, nxt = next_observed(iter, nout, last);
                CHECK(nxt > iter && nxt <= last && (nxt % nout == 0 || nxt == last));
                for (int64_t hb = 0; hb <= 1; hb++) CHECK(unobserved_run(iter, nout, last, hb) == by_hand(iter, nout, iterMax, hb));
                CHECK(observes_next(iter, nout, last) == (unobserved_run(iter, nout, last) == 0));
                CHECK(observes_next(iter, nout, last) == ((iter + 1) % nout == 0 || iter + 1 >= last));
            }
}

// the replays of whole loops, by the arithmetic alone (what else gates a replay in a driver -- convergence, a pending stress sweep -- is the driver's)
static void stokes_walks()
{
    const Walk vep = walk(299, 150, 32, 0, 1);        // 148 = 4 x 32 + 20, 149 = 4 x 32 + 21
    CHECK(vep.replays == 8 && vep.observed == 2 && vep.replays * 32 + vep.singles + vep.observed == 300);
    const Walk nl = walk(299, 100, 16, 0, 2);         // 97 = 6 x 16 + 1, 99 = 6 x 16 + 3, twice
    CHECK(nl.replays == 18 && nl.observed == 3 && nl.replays * 16 + nl.singles + nl.observed == 300);
    const Walk cx = walk(399, 200, 32, 1, 2);         // 196 = 6 x 32 + 4, 198 = 6 x 32 + 6
    CHECK(cx.replays == 12 && cx.observed == 2 && cx.replays * 32 + cx.singles + cx.observed == 400);
    CHECK(walk(40, 1, 32, 0, 1).replays == 0 && walk(40, 1, 32, 0, 1).observed == 41);
}

// the heat loop through the forwards of heat_plan.hpp: the cadences of tests/host/heat_plan_harness.cpp
static void heat_forwards()
{
    struct { int64_t iterMax, nout, unobserved, graphs, singles; } const known[] = {
        {45, 20, 42, 0, 42}, {70, 7, 60, 0, 60}, {99, 33, 96, 3, 0}, {300, 100, 297, 9, 9}, {102, 34, 99, 3, 3}, {4000, 1000000000, 3999, 124, 31},
        {1, 1, 0, 0, 0}, {1, 5, 0, 0, 0}, {40, 1, 0, 0, 0}, {10, 50, 9, 0, 9}, {33, 50, 32, 1, 0}, {34, 50, 33, 1, 1},
    };
    for (const auto &k : known) {
        int64_t iter = 0, unobserved = 0, graphs = 0, singles = 0;
        while (iter < k.iterMax) {
            int64_t run = heat_plan::unobserved_run(iter, k.nout, k.iterMax);
            CHECK(run == unobserved_run(iter, k.nout, k.iterMax) && heat_plan::next_observed(iter, k.nout, k.iterMax) == next_observed(iter, k.nout, k.iterMax));
            CHECK(heat_plan::observes_next(iter, k.nout, k.iterMax) == (run == 0));
            if (run >= heat_plan::kGraphIters) {
                for (; run >= heat_plan::kGraphIters; run -= heat_plan::kGraphIters) { iter += heat_plan::kGraphIters; graphs++; unobserved += heat_plan::kGraphIters; }
                continue;
            }
            if (run > 0) { unobserved++; singles++; }
            iter++;
        }
        CHECK(iter == k.iterMax && unobserved == k.unobserved && graphs == k.graphs && singles == k.singles);
    }
    CHECK(heat_plan::next_observed(0, 20, 45) == 20 && heat_plan::next_observed(19, 20, 45) == 20 && heat_plan::next_observed(20, 20, 45) == 40 &&
          heat_plan::next_observed(40, 20, 45) == 45 && heat_plan::next_observed(44, 20, 45) == 45);
}

int main()
{
    stokes_windows();
    stokes_walks();
    heat_forwards();
    printf("ok\n");
    return 0;
}
