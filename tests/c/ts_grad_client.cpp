// Stand-alone host program over csrc/ts_device.h (SPX_TS_HOST): reads one reduced phase r per line as a C99 hex float and prints
// sin2pi(r) of that header's own text as a hex float, once through sin2pi<1> and once as entry 2 of sin2pi<4> (the width the
// kernel uses: the value and its sign bit do not depend on it).  tests/test_ts_grad_host.py holds the output to
// tests/golden/ts_sin_mp.npz.
#define SPX_TS_HOST
#include "../../spearmint_amd/csrc/ts_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main()
{
    char buf[128];
    while (fgets(buf, sizeof buf, stdin)) {
        const double r = strtod(buf, nullptr);
        double a[1] = {r}, s1[1];
        sin2pi<1>(a, s1);
        double b[4] = {0.1, -0.3, r, 0.25}, s4[4];
        sin2pi<4>(b, s4);
        const bool same = memcmp(&s1[0], &s4[2], sizeof(double)) == 0 || (s1[0] != s1[0] && s4[2] != s4[2]);
        printf("%a %d\n", s1[0], (int)same);
    }
    return 0;
}
