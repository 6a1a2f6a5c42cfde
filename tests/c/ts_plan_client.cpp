// Stand-alone host program over csrc/spx_plan.h alone (no HIP, no library): plan_ts, what spx_thompson holds and whether it
// refuses for size.  One case per line from stdin, "N M D H S F per_draw"; one JSON line per case (tests/test_ts_host.py).
#include <stdio.h>

#include "../../spearmint_amd/csrc/spx_plan.h"

int main()
{
    long long N, M;
    int D, H, S, F, per_draw;
    while (scanf("%lld %lld %d %d %d %d %d", &N, &M, &D, &H, &S, &F, &per_draw) == 7) {
        TsShape s;
        s.N = N; s.M = M; s.Np = (int)round_up(N, SPX_PADN); s.D = D; s.H = H; s.S = S; s.F = F; s.per_draw = per_draw != 0;
        const TsPlan p = plan_ts(s);
        printf("{\"Mp\": %lld, \"Dp\": %d, \"sblocks\": %d, \"par_doubles\": %zu, \"w_bytes\": %zu, \"eps_bytes\": %zu, "
               "\"obs_bytes\": %zu, \"gamma_bytes\": %zu, \"path_bytes\": %zu, \"fits\": %d}\n",
               (long long)p.Mp, p.Dp, p.sblocks, p.par_doubles, p.w_bytes, p.eps_bytes, p.obs_bytes, p.gamma_bytes, p.path_bytes,
               (int)p.fits);
    }
    return 0;
}
