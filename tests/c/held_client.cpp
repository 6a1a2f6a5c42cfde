// Stand-alone host program over csrc/spx_held.h alone (no HIP, no library, no handle): reads one operation per line from
// stdin, applies it to the state the line gives and prints the state that results (tests/test_held.py).
//   BITS ATTRS drop THING
//   BITS ATTRS set THING [NEW_ATTRS]
// BITS: what is held, bit (1 << THING) per thing, THING the number of Held::Thing in its order of declaration.  ATTRS: the
// result attributes, bit 0 time_only, 1 moments, 2 tmean, 3 con, 4 global2d.  Output: "BITS ATTRS OK", OK = 0 where set refused.
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../../spearmint_amd/csrc/spx_held.h"

static Held::Results attrs_of(unsigned a)
{
    Held::Results r;
    r.time_only = a & 1; r.moments = a & 2; r.tmean = a & 4; r.con = a & 8; r.global2d = a & 16;
    return r;
}
static unsigned attrs_in(const Held::Results& r)
{
    return (r.time_only ? 1u : 0u) | (r.moments ? 2u : 0u) | (r.tmean ? 4u : 0u) | (r.con ? 8u : 0u) | (r.global2d ? 16u : 0u);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned bits = 0, attrs = 0, new_attrs = 0;
        int thing = -1;
        std::string op;
        if (!(in >> bits >> attrs >> op >> thing)) continue;
        in >> new_attrs;
        if (thing < 0 || thing >= Held::COUNT || bits >> Held::COUNT || attrs >> 5 || new_attrs >> 5) {
            fprintf(stderr, "held_client: bad line '%s'\n", line.c_str());
            return 2;
        }
        Held h;
        h.bits = bits;
        h.results = attrs_of(attrs);
        bool ok = true;
        if (op == "drop") h.drop((Held::Thing)thing);
        else if (op == "set") ok = h.set((Held::Thing)thing, attrs_of(new_attrs));
        else { fprintf(stderr, "held_client: unknown operation '%s'\n", op.c_str()); return 2; }
        printf("%u %u %d\n", (unsigned)h.bits, attrs_in(h.results), ok ? 1 : 0);
    }
    return 0;
}
