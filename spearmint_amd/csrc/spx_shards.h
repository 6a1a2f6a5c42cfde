// Who holds what on a multi-device handle: the shards of the candidates, of the hyper-parameter draws and of a log-likelihood
// batch over n device slots, as values.  Host-only, plain C++17: no HIP, no handle -- spx_multi.hip keeps one of each and
// replaces it whole, tests/c/shards_client.cpp runs the header on a CPU (tests/test_shards.py).  Every function here is a pure
// function of sizes.
//
// The slots form a ph x pc grid (spx_set_partition; ph = 1: candidates only): slot i evaluates the draws of hyper shard i % ph
// for the candidates of shard i / ph.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

// part r of `parts` contiguous parts of [0, total): equal, the first total % parts of them one longer
inline void shard(int64_t total, int parts, int r, int64_t* lo, int64_t* hi)
{
    const int64_t base = total / parts, extra = total % parts;
    *lo = r * base + (r < extra ? r : extra);
    *hi = *lo + base + (r < extra ? 1 : 0);
}

// slot i owns rows [lo[i], hi[i]) of the caller's M candidates; with fewer candidates than candidate shards the last shards
// are idle (on[i] = 0, an empty range at M).  `active` counts the slots that hold candidates.
struct CandShards {
    int64_t M = 0, index_base = 0;
    int active = 0;
    std::vector<int64_t> lo, hi;
    std::vector<char> on;
};

inline CandShards plan_cands(int n, int ph, int64_t M, int64_t index_base)
{
    CandShards c;
    c.M = M; c.index_base = index_base;
    c.lo.assign(n, M); c.hi.assign(n, M); c.on.assign(n, 0);
    const int used = (int)std::min<int64_t>(n / ph, M);
    for (int i = 0; i < n; ++i)
        if (i / ph < used) { shard(M, used, i / ph, &c.lo[i], &c.hi[i]); c.on[i] = 1; ++c.active; }
    return c;
}

// slot i holds the draws [hlo[i], hhi[i]) of the H of each model: all of them (ph = 1) or shard i % ph of ph
struct DrawShards {
    int H = 0;
    std::vector<int64_t> hlo, hhi;
    int count(int i) const { return (int)(hhi[i] - hlo[i]); }
};

inline DrawShards no_draws(int n)
{
    DrawShards d;
    d.hlo.assign(n, 0); d.hhi.assign(n, 0);
    return d;
}

// false (nothing written): fewer draws than hyper shards, or none
inline bool plan_draws(int n, int ph, int H, DrawShards* out)
{
    if (H < 1 || H < ph) return false;
    DrawShards d;
    d.H = H;
    d.hlo.assign(n, 0); d.hhi.assign(n, H);
    for (int i = 0; i < n; ++i) shard(H, ph, i % ph, &d.hlo[i], &d.hhi[i]);
    *out = d;
    return true;
}

// slot i's local index of objective draw `draw`, or -1
inline int local_draw(const DrawShards& d, int i, int32_t draw)
{
    return (draw >= d.hlo[i] && draw < d.hhi[i]) ? (int)(draw - d.hlo[i]) : -1;
}

// A slot numbers the draws it holds 0 .. count-1 (objective model), count .. 2 count-1 (time model); the handle numbers them
// 0 .. H-1 and H .. 2H-1.  The slots 0 .. ph-1 (candidate shard 0) hold every draw between them.
// global -> (slot of candidate shard 0, local); false: out of range
inline bool owner_of_draw(const DrawShards& d, int ph, int32_t draw, int* slot, int* local)
{
    const bool tm = draw >= d.H;
    const int32_t g = tm ? draw - d.H : draw;
    if (draw < 0 || g >= d.H) return false;
    for (int i = 0; i < ph; ++i) {
        const int l = local_draw(d, i, g);
        if (l >= 0) { *slot = i; *local = l + (tm ? d.count(i) : 0); return true; }
    }
    return false;
}
// (slot, local) -> global
inline int global_draw(const DrawShards& d, int slot, int local)
{
    const int c = d.count(slot);
    return local >= c ? d.H + (int)d.hlo[slot] + (local - c) : (int)d.hlo[slot] + local;
}

// The draws of a log-likelihood batch are independent: spx_gp_logprob shards them over min(n, H) slots, slot i < parts taking
// [lo[i], lo[i + 1]).  parts > 0 says that the slots hold these shards INSTEAD of the broadcast draws.
struct LogprobShards {
    int parts = 0;
    std::vector<int64_t> lo;        // parts + 1 bounds
    bool empty() const { return parts == 0; }
};

inline LogprobShards plan_logprob(int n, int H)
{
    LogprobShards s;
    s.parts = std::min(n, H);
    s.lo.assign(s.parts + 1, H);
    for (int i = 0; i < s.parts; ++i) { int64_t hi; shard(H, s.parts, i, &s.lo[i], &hi); }
    return s;
}
