// Stand-alone host program over csrc/kg_device.h (SPX_KG_HOST; built with -ffp-contract=off): reads line sets until the input ends,
// each "n" followed by n pairs "mu b", every number a C99 hex float (line 0 first), and prints the header's own knowledge gradient
// of every set as a hex float -- both sweeps over every line, then the terms added in the order of the lines, as k_kg_value does
// (tests/test_kg_host.py holds the output to tests/kg_oracle.py and tests/golden/kg_mp.npz).
#define SPX_KG_HOST
#include "../../spearmint_amd/csrc/kg_device.h"
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
    double nn = 0;
    while (next_number(nn)) {
        if (nn < 1 || nn > 256) return 2;
        const int n = (int)nn;
        std::vector<double> a(n), b(n);
        std::vector<unsigned char> on(n);
        bool bad = false;
        for (int i = 0; i < n; ++i) {
            if (!next_number(a[i]) || !next_number(b[i])) return 2;
            bad = bad || !std::isfinite(a[i]) || !std::isfinite(b[i]);
        }
        if (bad) { printf("%a\n", (double)NAN); continue; }
        for (int i = 0; i < n; ++i) on[i] = kg_on_envelope(a[0], a.data(), b.data(), 1, n, i) ? 1 : 0;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc = acc + (on[i] ? kg_term(a[0], a.data(), b.data(), 1, on.data(), 1, n, i) : 0.0);
        printf("%a\n", acc);
    }
    return 0;
}
