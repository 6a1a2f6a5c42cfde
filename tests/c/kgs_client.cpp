// Stand-alone host program over csrc/kg_fant_device.h (SPX_KG_HOST, -ffp-contract=off) with the 16-bit line indices of option
// "kg_scan" (KgsLines, n up to 1024): tests/c/kgf_client.cpp's input and output -- one row per set, the value as a hex float, then
// the n line indices in rank order (tests/test_kg_scan_host.py).
#define SPX_KG_HOST
#include "../../spearmint_amd/csrc/kg_fant_device.h"
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
        if (nn < 1 || nn > 1024) return 2;
        const int n = (int)nn;
        std::vector<double> a(n), b(n), bs(n);
        std::vector<unsigned short> perm(n);
        std::vector<unsigned> stk((n + 31) / 32);
        bool bad = false;
        for (int i = 0; i < n; ++i) {
            if (!next_number(a[i]) || !next_number(b[i])) return 2;
            bad = bad || !std::isfinite(a[i]) || !std::isfinite(b[i]);
        }
        for (int i = 0; i < n; ++i) {
            const int r = bad ? i : kgf_rank(b.data(), 1, n, i);
            perm[r] = (unsigned short)i;
            bs[r] = b[i];
        }
        const KgsLines L = {a[0], a.data() + 1, 1, perm.data(), 1, bs.data(), 1};    // (line p >= 1 reads mua[p - 1])
        const double v = bad ? (double)NAN : kgf_value(L, n, stk.data(), 1);
        printf("%a", v);
        for (int i = 0; i < n; ++i) printf(" %d", (int)perm[i]);
        printf("\n");
    }
    return 0;
}
