"""csrc/spx_shards.h on a CPU: who holds which candidates and which draws on a multi-device handle, and the two numberings of
the draws.  The header is run by tests/c/shards_client.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/plan_helpers.py).  Every expected value here is a literal or a closed form written in
this file, none is asked of the code under test."""
import pytest

from tests import plan_helpers as ph

pytestmark = pytest.mark.skipif(ph.compiler() is None, reason="no host C++ compiler")

GRIDS = [(n, p) for n in (1, 2, 3, 4, 6, 8) for p in range(1, n + 1) if n % p == 0]       # (slots, hyper shards)


def ask(lines):
    out = [[int(v) for v in ln.split()] for ln in ph.ask("shards_client", "".join(ln + "\n" for ln in lines))]
    assert len(out) == len(lines)
    return out


def part(total, parts, r):
    """Part r of `parts` contiguous parts of [0, total): equal, the first total % parts of them one longer."""
    lo = r * (total // parts) + min(r, total % parts)
    return lo, lo + total // parts + (1 if r < total % parts else 0)


def test_literals():
    got = ask(["cands 4 2 130 7", "cands 3 1 2 0", "cands 8 2 2147483653 0", "draws 4 2 5", "draws 4 2 1", "draws 2 1 0",
               "logprob 4 10", "logprob 6 2", "owner 4 2 5 3", "owner 4 2 5 8", "global 4 2 5 1 2", "owner 4 2 5 10", "owner 4 2 5 -1"])
    assert got[0] == [130, 7, 4, 0, 65, 1, 0, 65, 1, 65, 130, 1, 65, 130, 1]
    assert got[1] == [2, 0, 2, 0, 1, 1, 1, 2, 1, 2, 2, 0]                       # the third slot is idle: an empty range at M
    b = [0, 536870914, 1073741827, 1610612740, 2147483653]
    assert got[2] == [2147483653, 0, 8] + [v for i in range(8) for v in (b[i // 2], b[i // 2 + 1], 1)]
    assert got[3] == [1, 0, 3, 3, 5, 0, 3, 3, 5]                                # draws [0, 3) on slots 0, 2 and [3, 5) on 1, 3
    assert got[4] == [0] and got[5] == [0]
    assert got[6] == [4, 0, 3, 6, 8, 10] and got[7] == [2, 0, 1, 2]
    assert got[8] == [1, 1, 0]              # objective draw 3: slot 1's first
    assert got[9] == [1, 1, 2]              # draw 8 = time-model draw 3: behind slot 1's two objective draws
    assert got[10] == [8]
    assert got[11] == [0, -1, -1] and got[12] == [0, -1, -1]


@pytest.mark.parametrize("n,p", GRIDS)
def test_candidate_shards_partition_the_candidates(n, p):
    Ms = sorted({M for M in (1, 2, n - 1, n, n + 1, 130, 2 ** 31 + 5) if M >= 1})
    for M, got in zip(Ms, ask(["cands %d %d %d 11" % (n, p, M) for M in Ms])):
        assert got[:2] == [M, 11] and len(got) == 3 + 3 * n
        slots = [tuple(got[3 + 3 * i:6 + 3 * i]) for i in range(n)]
        used = min(n // p, M)                                   # candidate shards that hold rows
        assert got[2] == used * p                               # active: every slot of those shards
        for j in range(p):                                      # the slots of draw shard j, one per candidate shard
            col = slots[j::p]
            assert [s[2] for s in col] == [1] * used + [0] * (n // p - used), (M, j, col)
            assert all((lo, hi) == (M, M) for lo, hi, on in col[used:])
            end = 0
            for r, (lo, hi, on) in enumerate(col[:used]):       # in order, disjoint, nothing left out
                assert lo == end and hi > lo, (M, j, col)
                assert (lo, hi) == part(M, used, r)
                end = hi
            assert end == M


@pytest.mark.parametrize("n,p", GRIDS)
def test_draw_shards_partition_the_draws(n, p):
    Hs = list(range(0, 2 * p + 2))
    for H, got in zip(Hs, ask(["draws %d %d %d" % (n, p, H) for H in Hs])):
        if H < p or H < 1:
            assert got == [0], (H, got)
            continue
        assert got[0] == 1 and len(got) == 1 + 2 * n
        slots = [tuple(got[1 + 2 * i:3 + 2 * i]) for i in range(n)]
        assert slots == [part(H, p, i % p) for i in range(n)]
        end = 0
        for lo, hi in slots[:p]:                                # candidate shard 0 holds every draw, in order
            assert lo == end and hi > lo
            end = hi
        assert end == H


@pytest.mark.parametrize("n,p", GRIDS)
def test_the_two_numberings_of_the_draws_are_inverse(n, p):
    for H in (p, p + 1, 2 * p + 1):
        want = {}                                               # handle's number -> (slot, slot's number), both models
        for j in range(p):
            lo, hi = part(H, p, j)
            for model in (0, 1):
                for d in range(lo, hi):
                    want[model * H + d] = (j, model * (hi - lo) + d - lo)
        assert sorted(want) == list(range(2 * H))
        gs = sorted(want)
        owners = ask(["owner %d %d %d %d" % (n, p, H, g) for g in gs + [-1, 2 * H]])
        assert owners[-2][0] == 0 and owners[-1][0] == 0
        assert [tuple(o) for o in owners[:-2]] == [(1,) + want[g] for g in gs]
        back = ask(["global %d %d %d %d %d" % ((n, p, H) + want[g]) for g in gs])
        assert [b[0] for b in back] == gs


def test_logprob_shards():
    cases = [(n, H) for n in (1, 2, 3, 4, 6, 8) for H in (1, 2, n - 1, n, n + 1, 17) if H >= 1]
    for (n, H), got in zip(cases, ask(["logprob %d %d" % c for c in cases])):
        parts = min(n, H)
        assert got == [parts] + [part(H, parts, r)[0] for r in range(parts)] + [H]
