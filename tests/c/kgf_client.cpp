// Stand-alone host program over csrc/kg_fant_device.h (SPX_KG_HOST, -ffp-contract=off): tests/c/kg_client.cpp's input; one row per
// set: the header's knowledge gradient as a hex float -- rank counting, the scan, the term walk, as k_kgf_order and k_kgf_value run
// them -- then the n line indices in rank order (tests/test_kg_pending_host.py).
#define SPX_KG_HOST
#include "../../spearmint_amd/csrc/kg_fant_device.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static bool next_number(double& x)
{
    char buf[128];
    const bool ok = scanf("%127s", buf) == 1;
    if (ok) x = strtod(buf, nullptr);
    return ok;
}

int main()
{
    double nn = 0;
    while (next_number(nn)) {
        if (nn < 1 || nn > 256) return 2;
        const int n = (int)nn;
        std::vector<double> a(n), b(n), bs(n);
        std::vector<unsigned char> perm(n);
        std::vector<unsigned> stk((n + 31) / 32);
        bool bad = false;
        for (int i = 0; i < n; ++i) {
            if (!next_number(a[i]) || !next_number(b[i])) return 2;
            bad = bad || !std::isfinite(a[i]) || !std::isfinite(b[i]);
        }
        for (int i = 0; i < n; ++i) {
            const int r = bad ? i : kgf_rank(b.data(), 1, n, i);
            perm[r] = (unsigned char)i;
            bs[r] = b[i];
        }
        const KgfLines L = {a[0], a.data() + 1, 1, perm.data(), 1, bs.data(), 1};    // (line p >= 1 reads mua[p - 1])
        const double v = bad ? (double)NAN : kgf_value(L, n, stk.data(), 1);
        printf("%a", v);
        for (int i = 0; i < n; ++i) printf(" %d", (int)perm[i]);
        printf("\n");
    }
    return 0;
}
