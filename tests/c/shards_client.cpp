// Stand-alone host program over csrc/spx_shards.h alone (no HIP, no library, no handle): reads one question per line from stdin
// and prints one line of integers per question (tests/test_shards.py).
//   cands N PH M BASE        -> M BASE ACTIVE, then LO HI ON for each of the N slots
//   draws N PH H             -> OK (0: refused, nothing else), then HLO HHI for each slot
//   owner N PH H DRAW        -> OK SLOT LOCAL           (handle's numbering -> a slot of candidate shard 0 and its numbering)
//   global N PH H SLOT LOCAL -> DRAW                    (and back)
//   logprob N H              -> PARTS, then the PARTS + 1 bounds
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../../spearmint_amd/csrc/spx_shards.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q;
        long long a[5] = {0, 0, 0, 0, 0};
        if (!(in >> q)) continue;
        int na = 0;
        while (na < 5 && (in >> a[na])) ++na;
        const int n = (int)a[0], ph = (int)a[1];
        DrawShards d;
        if (q == "cands" && na == 4 && n >= 1 && ph >= 1 && n % ph == 0) {
            const CandShards c = plan_cands(n, ph, a[2], a[3]);
            printf("%lld %lld %d", (long long)c.M, (long long)c.index_base, c.active);
            for (int i = 0; i < n; ++i) printf(" %lld %lld %d", (long long)c.lo[i], (long long)c.hi[i], (int)c.on[i]);
            printf("\n");
        } else if (q == "draws" && na == 3 && n >= 1 && ph >= 1 && n % ph == 0) {
            const bool ok = plan_draws(n, ph, (int)a[2], &d);
            printf("%d", ok ? 1 : 0);
            for (int i = 0; ok && i < n; ++i) printf(" %lld %lld", (long long)d.hlo[i], (long long)d.hhi[i]);
            printf("\n");
        } else if (q == "owner" && na == 4 && plan_draws(n, ph, (int)a[2], &d)) {
            int slot = -1, local = -1;
            const bool ok = owner_of_draw(d, ph, (int32_t)a[3], &slot, &local);
            printf("%d %d %d\n", ok ? 1 : 0, slot, local);
        } else if (q == "global" && na == 5 && plan_draws(n, ph, (int)a[2], &d) && a[3] >= 0 && a[3] < n && a[4] >= 0) {
            printf("%d\n", global_draw(d, (int)a[3], (int)a[4]));
        } else if (q == "logprob" && na == 2 && n >= 1 && a[1] >= 1) {
            const LogprobShards s = plan_logprob(n, (int)a[1]);
            printf("%d", s.parts);
            for (int64_t b : s.lo) printf(" %lld", (long long)b);
            printf("\n");
        } else {
            fprintf(stderr, "shards_client: bad line '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
