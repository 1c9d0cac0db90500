// vep3_plan_harness.cpp -- known answers for csrc/vep3_plan.hpp (the launch plan of the 3D VEP driver), built with g++ under -fsanitize=address,undefined
// (tests/test_host_vep3_plan.py).  The answers were computed from the expressions the driver held before the plan existed: the thresholds (125,000 nodes, 3,000 blocks,
// 62-column segments, rem <= 24, 2,048 blocks, 16,384 node columns) are pinned on both of their sides.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "vep3_plan.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// defaults: two phases, no softening law, called by the solve loop, "vep3_edges" = 4, "vep3_cfg" = 0, "vep3_peel" = 1
static Vep3EdgePlan plan(int nx, int ny, int nz, int nphase = 2, bool soft = false, bool loop = true, int edges = 4, int cfg = 0, bool peel = true)
{
    return vep3_plan_edges(nx, ny, nz, nphase, soft, loop, edges, cfg, peel);
}

static void node_form()
{
    CHECK(plan(49, 49, 49).form == 0 && !plan(49, 49, 49).refused);      // 50^3 = 125,000 is still "<="
    CHECK(plan(3, 3, 3).form == 0 && plan(48, 48, 48).form == 0 && plan(125, 6, 18).form == 0);
    const Vep3EdgePlan s = plan(3, 3, 3, 2, false, false);               // the kernel-level entry point keeps the form the switch names
    CHECK(!s.refused && s.form == 4 && s.kz == 4);
    CHECK(plan(256, 256, 256, 5).form == 0 && plan(3, 3, 3, 5, false, false).form == 0 && !plan(256, 256, 256, 5).refused);      // more than four phases: at any size
    CHECK(plan(256, 256, 256, 2, false, true, 0).form == 0);
}

static void form_4()
{
    Vep3EdgePlan p = plan(50, 49, 49);
    CHECK(!p.refused && p.form == 4 && p.kz == 4);
    p = plan(56, 56, 56);
    CHECK(p.form == 4 && p.kz == 4 && !p.peel && p.nseg == 1 && p.ilim == 57 && p.nzc == 15);
    p = plan(64, 64, 64);
    CHECK(p.form == 4 && p.kz == 4 && p.nseg == 2 && p.ilim == 65 && p.nzc == 17);
    p = plan(128, 128, 128);
    CHECK(p.form == 4 && p.kz == 8 && p.peel && p.rem == 5 && p.nseg == 2 && p.ilim == 124 && p.nzc == 17);
    CHECK(p.peel_gx == (5u * 129u + 63u) / 64u && p.peel_gy == (129u + 3u) / 4u);
    p = plan(160, 160, 160);
    CHECK(p.form == 4 && p.kz == 16 && !p.peel && p.nseg == 3 && p.ilim == 161 && p.nzc == 11);
    p = plan(256, 256, 256);
    CHECK(p.form == 4 && p.kz == 16 && p.peel && p.rem == 9 && p.nseg == 4 && p.ilim == 248 && p.nzc == 17);
    CHECK(p.ntxy == 260 && p.ntxy_l == 1028 && p.nt == 260 * 17 && p.nt_l == 1028 * 17);
    CHECK(p.grid_l == 17480u && p.grid_f == 4424u * 3u);                 // 17,476 and 4,420 tiles, padded to whole rounds of 8
    p = plan(256, 256, 256, 2, false, true, 4, 0, false);                // "vep3_peel" = 0
    CHECK(!p.peel && p.nseg == 5 && p.ilim == 257);
    p = plan(200, 96, 70);
    CHECK(p.form == 4 && p.kz == 4 && p.peel && p.rem == 15 && p.nseg == 3 && p.ilim == 186 && p.nzc == 18);
    p = plan(147, 40, 40);                                               // rem = 24 is the last peeled value
    CHECK(p.form == 4 && p.peel && p.rem == 24 && p.nseg == 2 && p.ilim == 124);
    p = plan(148, 40, 40);
    CHECK(p.form == 4 && !p.peel && p.nseg == 3 && p.ilim == 149);
    p = plan(126, 127, 200);
    CHECK(p.form == 4 && p.kz == 16 && p.nseg == 2 && p.nzc == 13);
    for (int cfg : {162, 82, 42}) CHECK(!plan(256, 256, 256, 2, false, true, 4, cfg).refused && plan(256, 256, 256, 2, false, true, 4, cfg).kz == cfg / 10);
    CHECK(plan(256, 256, 256, 2, false, true, 4, 322).refused && plan(256, 256, 256, 2, false, true, 4, 22).refused);
}

static void other_forms_and_refusals()
{
    Vep3EdgePlan p = plan(256, 256, 256, 2, false, true, 1, 82);
    CHECK(!p.refused && p.form == 1 && p.kz == 8 && p.mb == 2 && p.nzc == 33);
    for (int cfg : {0, 162, 163, 82}) CHECK(!plan(256, 256, 256, 2, false, true, 1, cfg).refused);
    for (int cfg : {83, 42, 164, 161}) CHECK(plan(256, 256, 256, 2, false, true, 1, cfg).refused);
    for (int edges : {2, 3, 6}) {
        p = plan(256, 256, 256, 2, false, true, edges);
        CHECK(!p.refused && p.form == edges && p.kz == 16);
        p = plan(64, 64, 64, 2, false, true, edges);                     // only form 4 halves its chunks
        CHECK(!p.refused && p.form == edges && p.kz == 16);
        p = plan(256, 256, 256, 2, false, true, edges, 82);
        CHECK(p.refused && strcmp(p.refused, "vep3_cfg: no such configuration") == 0);
    }
    // softening laws: 16 planes, not halved
    p = plan(256, 256, 256, 2, true);
    CHECK(!p.refused && p.form == 1 && p.kz == 16 && p.mb == 2);
    p = plan(64, 64, 64, 2, true);
    CHECK(!p.refused && p.kz == 16);
    p = plan(256, 256, 256, 2, true, true, 4, 82);
    CHECK(p.refused && strcmp(p.refused, "vep3_cfg: no such configuration") == 0);
    CHECK(plan(49, 49, 49, 2, true).form == 0);
    for (int edges : {5, 7, -1}) {
        p = plan(256, 256, 256, 2, false, true, edges);
        CHECK(p.refused && strcmp(p.refused, "vep3_edges: no such form") == 0);
        p = plan(256, 256, 256, 2, true, false, edges);
        CHECK(p.refused && strcmp(p.refused, "vep3_edges: no such form") == 0);
        CHECK(plan(3, 3, 3, 5, false, true, edges).refused);             // also where the node kernel would have run
    }
}

static void prekz()
{
    const int want[7][4] = {{16, 16, 16, 1}, {96, 96, 96, 1}, {200, 96, 70, 2}, {128, 128, 128, 4}, {126, 127, 200, 4}, {160, 160, 160, 8}, {256, 256, 256, 8}};
    for (const int *w : want) CHECK(vep3_plan_prekz(w[0], w[1], w[2], 0) == w[3]);
    for (int forced : {1, 2, 3, 4, 8, 16, 32}) CHECK(vep3_plan_prekz(16, 16, 16, forced) == forced && vep3_plan_prekz(256, 256, 256, forced) == forced);
    for (int kz : {1, 2, 4, 8, 16, 32}) CHECK(vep3_pre_depth(kz) == kz);
    CHECK(vep3_pre_depth(3) == 8 && vep3_pre_depth(64) == 8);
}

static void prec_map()
{
    Vep3PrecPlan p = vep3_plan_prec(127, 127, 127, 8, 2);               // 128 * 128 = 16,384 node columns: tiled
    CHECK(p.tntx == 2 && p.gx == 2u * 32u && p.gy == 16u && p.kz == 8);
    p = vep3_plan_prec(126, 127, 127, 8, 2);
    CHECK(p.tntx == 0 && p.gx == (127u * 128u + 255u) / 256u && p.gy == 16u);
    p = vep3_plan_prec(126, 127, 127, 4, 1);
    CHECK(p.tntx == 2 && p.gx == 64u && p.gy == 32u);
    p = vep3_plan_prec(127, 127, 127, 1, 0);
    CHECK(p.tntx == 0 && p.gx == 64u && p.gy == 128u);
    p = vep3_plan_prec(256, 256, 256, 8, 2);
    CHECK(p.tntx == 5 && p.gx == 5u * 65u && p.gy == 33u);
}

int main()
{
    node_form();
    form_4();
    other_forms_and_refusals();
    prekz();
    prec_map();
    printf("ok\n");
    return 0;
}
