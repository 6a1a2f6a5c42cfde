"""Dev tool: do spx_ei_grad_batch and spx_constrained_ei_grad_batch return the same BITS with the in-tree libspx.so and with
other builds of it (paths given, e.g. one built from the parent commit's sources in a directory outside the tree)?
   python scripts/dev/refine_bits_ab.py /somewhere/libspx_parent.so [...]
Every library runs in a child process of its own (Engine(0, lib=...)), which prints one sha256 per case over the raw bytes
of f and grad; the cases are single-axis departures from a small base, through every branch of both entry points.  A child
that fails or runs out of time ends the run there."""
import os, sys, subprocess, json, hashlib
here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
CHILD_TIMEOUT_S = 240

BASE = dict(N=40, D=3, H=2, P=9, S=4, covar="Matern52")
AXES = (("N", (2, 64, 65, 255, 257, 300)),      # 64-row workgroups, 256-wide j chunks, 256-thread strides
        ("D", (1, 8, 9, 17)),                   # eight dimensions per gradient pass
        ("H", (1, 3)),
        ("P", (1, 8, 9, 21)),                   # eight right-hand sides share a pass over W
        ("S", (1, 4, 5, 100)),                  # four waves stride over the fantasies
        ("covar", ("Matern52", "Matern32", "ARDSE")))


def cases():
    out = [("base", BASE)]
    for key, values in AXES:
        out += [("%s=%s" % (key, v), dict(BASE, **{key: v})) for v in values if v != BASE[key]]
    return out


def child(lib):
    sys.path.insert(0, root)
    import numpy as np
    from spearmint_amd.engine import Engine
    from tests import refine_helpers as rh
    from tests import constrained_refine_helpers as hp

    def digest(f, g):
        return hashlib.sha256(np.ascontiguousarray(f).tobytes() + np.ascontiguousarray(g).tobytes()).hexdigest()

    def run(setup, p, call, P):
        eng = Engine(0, lib=None if lib == "-" else lib)
        try:
            setup(eng, p)
            return digest(*call(eng, hp.points(p, 11, P)))
        finally:
            eng.close()

    def constrained(c, seed, state, n_valid=None, n_full=None):
        fant = state.endswith("fant")
        n_pend = min(3, c["N"] - 1) if fant else 0
        n_valid = c["N"] - n_pend if n_valid is None else n_valid
        if n_full is None:
            n_full = n_valid + 10 if state.startswith("viol") else n_valid
        p = hp.make_problem(seed, c["covar"], D=c["D"], n_valid=n_valid, n_full=n_full, H=c["H"],
                            S=c["S"] if fant else 0, n_pend=n_pend)
        return run(hp.setup, p, lambda e, x: e.constrained_ei_grad_batch(x, p.best), c["P"])

    out = {}
    for k, (name, c) in enumerate(cases()):
        for branch in rh.BRANCHES:      # the plain entry: plain, per second, fantasies
            p = rh.make_problem(100 + k, c["covar"], branch, N=c["N"], D=c["D"], H=c["H"], S=c["S"])
            out["%s ei/%s" % (name, branch)] = run(rh.setup, p, lambda e, x: e.ei_grad_batch(x), c["P"])
        for state in ("nov", "nov_fant", "viol", "viol_fant"):     # the constrained entry: violation seen x fantasies
            out["%s cei/%s" % (name, state)] = constrained(c, 200 + k, state)
    for n_full in (40, 70):             # the two-factor path: the variance over the constraint model's points
        out["two-factor n_valid=30 n_full=%d cei/viol" % n_full] = constrained(BASE, 300 + n_full, "viol", 30, n_full)
    print(json.dumps(out))


if len(sys.argv) > 2 and sys.argv[1] == "--child":
    child(sys.argv[2])
    sys.exit(0)
libs = ["-"] + sys.argv[1:]
res = []
for lib in libs:
    try:
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib], stdout=subprocess.PIPE,
                           timeout=CHILD_TIMEOUT_S, check=True).stdout.decode().strip().splitlines()[-1]
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as ex:
        print("library %s: %s -- stopping here" % (lib, ex))
        sys.exit(2)
    res.append(json.loads(o))
print("libraries: in-tree" + "".join(", " + os.path.basename(l) for l in libs[1:]))
differing = 0
for key in res[0]:
    marks = ["same" if r[key] == res[0][key] else "DIFFERS" for r in res[1:]]
    differing += "DIFFERS" in marks
    print("%-44s %s  %s" % (key, res[0][key][:16], "  ".join(marks)))
print("%d cases, %d differing" % (len(res[0]), differing))
sys.exit(1 if differing else 0)
