// What a handle holds, and what each of those things was made from.  Host-only, plain C++17: no HIP, no handle -- spx_api.hip
// executes it for a single handle (spx_drop / spx_hold), spx_multi.hip for the front of a multi-device handle, which keeps a
// record of its own beside those of its per-device handles (multi_drop / multi_hold; CON, CON_FACTOR, FULL_FACTOR and ALPHA_S are
// never set there); tests/c/held_client.cpp runs it on a CPU (tests/test_held.py).
//
// One rule for every entry point: DROP what the call is about to overwrite before its first mutation, SET it after its last
// check.  Dropping a thing clears it and, transitively, everything made from it; a call that fails in between leaves what it
// was overwriting not held -- its readers refuse with their "call ... first" errors -- and everything it did not touch as it was.
#pragma once
#include <stdint.h>

// what the last EI pass kept; all false whenever RESULTS is not held
struct HeldResults {
    bool time_only = false;    // SPX_FLAG_TIME_ONLY: predicted durations only, no EI results
    bool moments = false;      // func_m / func_v (spx_get_moments)
    bool tmean = false;        // predicted durations (spx_get_time_mean)
    bool con = false;          // constraint probabilities (spx_get_constraint_prob)
    bool global2d = false;     // spx_get_ei_mean serves the all-reduced vector of a 2-D partition
    bool mes = false;          // the pass was a max-value entropy search: its y* table, fit and G are resident (spx_get_mes,
                               // spx_ei_grad_batch under SPX_ACQ_MES); gone with the results, so with everything that drops them
    bool ehvi = false;         // the pass was an expected-hypervolume-improvement pass: the second GP's func_m / func_v of the same
                               // candidates are resident on its internal handle (spx_get_moments, draws H .. 2H-1)
    bool ts = false;           // the "pass" was spx_thompson: what is resident are posterior sample paths and their priors
                               // (spx_get_thompson_path / _prior), a results kind of its own -- no EI values, no winner
    bool ts_alpha = false;     // ... and alpha = W^T Gamma of every held path is resident too (built by the first
                               // spx_thompson_grad_batch after a spx_thompson); gone with the paths, so with everything that drops them
    bool kg = false;           // the pass was a knowledge-gradient pass: mu_a of its representer points is resident
    bool kg_lines = false;     // ... and, kept with the moments, the covariances C[d][a][c] (spx_get_kg_lines)
};

struct Held {
    enum Thing {
        OBS, CAND, HYP, TIME, CON,                                   // inputs (spx_set_*)
        FACTOR, CON_FACTOR, FULL_FACTOR, FANT, ALPHA_S, RESULTS,     // products
        COVAR, PARTITION,   // never held: option "covar" / the communicator and the partition -- named so that the table can
                            // say what is made from them, and drop(COVAR) / drop(PARTITION) is what a change of either does
        // two objectives (SPX_ACQ_EHVI), numbered behind the two above so that nothing before them moves:
        FRONT,              // input: the Pareto front and its reference point (spx_set_pareto_front)
        SEC,                // product: the second GP's internal handle holds (comp, second values, second hypers)
        SEC_CAND,           // product: ... and the candidates
        // the knowledge gradient (SPX_ACQ_KG), behind those again:
        KGPTS,              // input: the representer points (spx_set_kg_points)
        COUNT
    };
    using Results = HeldResults;

    uint32_t bits = 0;
    Results results;

    bool has(Thing x) const { return (bits >> x) & 1u; }
    bool ei() const { return has(RESULTS) && !results.time_only && !results.ts; }   // EI results, not durations or paths only
    inline void drop(Thing x);                                        // clears x and everything made from it; never adds a bit
    inline bool set(Thing x, Results r = Results());                  // false (nothing changes): a thing x needs is not held
};

// "X is made from ...".  needs: set(X) is refused without them.  uses: read when X was made if they were held then (a factor
// with or without a time model, a pass with or without fantasies) -- they may be absent, but X does not survive their drop.
struct HeldRow { uint32_t needs, uses; };
#define SPX_HB(x) (1u << Held::x)
static constexpr HeldRow kHeldMadeFrom[Held::COUNT] = {
    /* OBS         */ {0, 0},
    /* CAND        */ {0, 0},
    /* HYP         */ {0, 0},
    /* TIME        */ {SPX_HB(OBS) | SPX_HB(HYP), 0},               // new observations or new hypers drop the time model
    /* CON         */ {0, 0},                                       // (its own points and hypers: spx_set_constraint_model)
    /* FACTOR      */ {SPX_HB(OBS) | SPX_HB(HYP), SPX_HB(TIME) | SPX_HB(COVAR)},
    /* CON_FACTOR  */ {SPX_HB(CON), SPX_HB(COVAR)},
    /* FULL_FACTOR */ {SPX_HB(OBS) | SPX_HB(HYP) | SPX_HB(CON), SPX_HB(COVAR)},
    /* FANT        */ {SPX_HB(FACTOR), 0},                          // S > 0 exactly when FANT is held
    /* ALPHA_S     */ {SPX_HB(FANT), 0},
    /* RESULTS     */ {SPX_HB(FACTOR) | SPX_HB(CAND), SPX_HB(FANT) | SPX_HB(CON) | SPX_HB(PARTITION) | SPX_HB(FRONT) | SPX_HB(KGPTS)},
    /* COVAR       */ {0, 0},
    /* PARTITION   */ {0, 0},
    /* FRONT       */ {0, 0},                                       // a new front drops the results of the last pass alone
    /* SEC         */ {SPX_HB(TIME), 0},                            // (option "covar" reaches the internal handle itself: it drops its own factor)
    /* SEC_CAND    */ {SPX_HB(CAND), 0},
    /* KGPTS       */ {0, 0},                                       // new points drop the results of the last pass alone
};
#undef SPX_HB

inline void Held::drop(Thing x)
{
    uint32_t gone = 1u << x;
    for (bool more = true; more;) {
        more = false;
        for (int t = 0; t < COUNT; ++t)
            if (!((gone >> t) & 1u) && ((kHeldMadeFrom[t].needs | kHeldMadeFrom[t].uses) & gone)) { gone |= 1u << t; more = true; }
    }
    bits &= ~gone;
    if (!has(RESULTS)) results = Results();
}

inline bool Held::set(Thing x, Results r)
{
    if (x == COVAR || x == PARTITION || x >= COUNT || (kHeldMadeFrom[x].needs & ~bits)) return false;
    bits |= 1u << x;
    if (x == RESULTS) results = r;
    return true;
}
