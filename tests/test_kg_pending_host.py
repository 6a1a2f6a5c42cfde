"""csrc/kg_fant_device.h -- rank counting, the stack scan, the term walk -- compiled for the host (tests/c/kgf_client.cpp, no
contraction, address and undefined-behaviour sanitizers) on the crafted line sets of tests/kg_mp.py: held to the 50-digit yardstick
at the plain header's bar, to the plain header's all-pairs value at two such bars (the two rules may differ by a line that touches
the envelope), its order to np.lexsort's.  GPU: tests/test_gpu_zx_kg_pending.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import kg_helpers as kh
from tests import kg_mp as km
from tests import plan_helpers as ph

_exe = []


def scan_on_host(sets):
    """(values, [line indices by rank]) of every (mu, b) from kg_fant_device.h on the host."""
    if not _exe:
        exe = os.path.join(tempfile.mkdtemp(prefix="spx_kgf_client_"), "kgf_client")
        subprocess.check_call([ph.compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                               os.path.join(ph.ROOT, "tests", "c", "kgf_client.cpp")])
        _exe.append(exe)
    text = []
    for mu, b in sets:
        text.append("%d\n" % len(mu))
        text += ["%s %s\n" % (float(m).hex(), float(s).hex()) for m, s in zip(mu, b)]
    rows = subprocess.run([_exe[0]], input="".join(text).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    rows = [r.split() for r in rows]
    return np.array([float.fromhex(r[0]) for r in rows]), [np.array(r[1:], dtype=int) for r in rows]


@pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")
def test_scan_against_50_digits_the_all_pairs_rule_and_lexsort(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "kg_mp.npz")))
    named = km.sets_of(fx)
    rng = np.random.RandomState(4)
    sets = [(mu, b) for _, mu, b in named]
    for n in (2, 3, 7, 17, 33, 65, 129, 256):              # random sets beside the crafted ones, as the plain header's test has
        sets.append((rng.randn(n) * rng.choice([1.0, 0.01]), rng.randn(n) * rng.choice([1.0, 1e-3, 50.0])))
    sets.append((np.arange(40.0) ** 2 / 40.0, -np.arange(40.0)))      # every line on the envelope: the stack at its deepest
    got, perms = scan_on_host(sets)
    assert got.shape == (len(sets),)
    kh.held_to_yardstick(fx, got, sets, "kg_fant_device.h on the host")
    plain = kh.device_header_on_host(sets)
    for k, (mu, b) in enumerate(sets):
        _, unit, band = kh.yardstick(mu, b)
        e = km.error(got[k:k + 1], plain[k:k + 1], np.array([unit]))
        assert e <= 2 * kh.MARGIN * km.pinned(fx, band), (k, got[k], plain[k])
        assert np.array_equal(perms[k], np.lexsort((np.arange(len(b)), -np.asarray(b)))), k
    by_name = {n: g for (n, _, _), g in zip(named, got)}
    for name in ("equal_slopes", "equal_slopes_zero", "rand_n1_0", "zero_slope_line0_alone", "far_40"):
        assert by_name[name] == 0.0 and not np.signbit(by_name[name]), name          # exactly +0.0
    assert np.all(got >= 0.0) and not np.any(np.signbit(got))
    # a non-finite line: NaN for that set alone, the order of the lines kept
    out, perm = scan_on_host([(np.array([0.0, np.nan, 1.0]), np.array([1.0, 0.5, 0.0])),
                              (np.array([0.0, 0.2, 1.0]), np.array([0.0, np.inf, 1.0])), sets[3]])
    assert np.all(np.isnan(out[:2])) and out[2] == got[3] and perm[1].tolist() == [0, 1, 2]

