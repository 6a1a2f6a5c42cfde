// Stand-alone host program over csrc/ts_device.h (SPX_TS_HOST): reads one reduced phase r per line as a C99 hex float and prints
// cos2pi(r) of that header's own text as a hex float, once through cos2pi<1> and once as entry 2 of cos2pi<4> (the width the
// kernel uses: the value does not depend on it).  tests/test_ts_host.py holds the output to tests/golden/ts_cos_mp.npz.
#define SPX_TS_HOST
#include "../../spearmint_amd/csrc/ts_device.h"
#include <cstdio>
#include <cstdlib>

int main()
{
    char buf[128];
    while (fgets(buf, sizeof buf, stdin)) {
        const double r = strtod(buf, nullptr);
        double a[1] = {r}, c1[1];
        cos2pi<1>(a, c1);
        double b[4] = {0.1, -0.3, r, 0.25}, c4[4];
        cos2pi<4>(b, c4);
        printf("%a %d\n", c1[0], (int)(c1[0] == c4[2] || (c1[0] != c1[0] && c4[2] != c4[2])));
    }
    return 0;
}
