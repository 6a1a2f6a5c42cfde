// Stand-alone host program over csrc/ehvi_device.h (SPX_EHVI_HOST; built with -ffp-contract=off): reads "nstrips ncand", then
// nstrips edges, nstrips levels and ncand rows m1 v1 m2 v2, every number a C99 hex float, and prints the header's own EHVI of
// every candidate as a hex float -- walked in tiles of TILE strips as k_ehvi walks them (tests/test_pareto_host.py holds the
// output to tests/ehvi_oracle.py on tests/golden/ehvi_mp.npz).
#define SPX_EHVI_HOST
#include "../../spearmint_amd/csrc/ehvi_device.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static bool next_number(double& x)
{
    char buf[128];
    if (scanf("%127s", buf) != 1) return false;
    x = strtod(buf, nullptr);
    return true;
}

int main()
{
    const int TILE = 256;
    double ns = 0, nc = 0;
    if (!next_number(ns) || !next_number(nc) || ns < 1 || ns > 4097 || nc < 0 || nc > 1e6) return 2;
    const int nstrips = (int)ns, ncand = (int)nc;
    std::vector<double> edges(nstrips), levels(nstrips);
    for (double& e : edges) if (!next_number(e)) return 2;
    for (double& l : levels) if (!next_number(l)) return 2;
    for (int c = 0; c < ncand; ++c) {
        double m1, v1, m2, v2;
        if (!next_number(m1) || !next_number(v1) || !next_number(m2) || !next_number(v2)) return 2;
        double g_lo = 0.0, acc = 0.0;
        for (int t0 = 0; t0 < nstrips; t0 += TILE)
            ehvi_strips(m1, v1, m2, v2, edges.data() + t0, levels.data() + t0, std::min(TILE, nstrips - t0), t0 == 0, g_lo, acc);
        printf("%a\n", acc);
    }
    return 0;
}
