"""Shared by tests/test_plan.py, tests/test_held.py, tests/test_shards.py (CPU) and tests/test_gpu_r_plan_runs.py: builds a client
under tests/c -- a stand-alone host program over one host-only header of csrc -- with the host C++ compiler and the address /
undefined-behaviour sanitizers, and asks it: plan_client.cpp for plans, held_client.cpp for what a handle holds,
shards_client.cpp for who holds what on a multi-device handle.  A case is ("factor" | "ei", {key: value}); keys are the shape's (plan_client.cpp) and option names."""
import json
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
_clients = {}


# The EI pass's acquisition decisions as plan_client prints them (the enums of csrc/spx_plan.h, SPX_ACQ_* of include/spx.h), and
# the rows tests/test_plan.py pins on the CPU and tests/test_gpu_r_plan_runs.py runs: N = 130 (128: the fused rows), M = 1000,
# H = 3, D = 2, A = 5 representer points, S = 3 fantasies / paths.
ACQ = {"EI": 0, "PI": 1, "LCB": 2, "MES": 3, "EHVI": 4, "KG": 5}
FINISH = {"fused": 0, "all_draws": 1, "per_fantasy": 2, "mes_fant_means": 3, "ts": 4, "kg_pairs": 5, "kg_scan": 6, "kgf_lines8": 7,
          "kgf_lines16": 8}
TAIL = {"none": 0, "mes": 1, "mes_fant": 2, "ehvi": 3, "kgf_value": 4, "kgw_value": 5}
CLOSING = {"mean_argmax": 0, "ts_argmin": 1}
RHS = {"fant": 0, "ts": 1, "kg": 2}
ACQ_A, ACQ_S, ACQ_K = 5, 3, 4
# name: (N, shape keys and options, (finish, tail, closing, pass_acq, keep_mom as the pass runs, rhs_S))
ACQ_ROWS = {}
for _a in ("EI", "PI", "LCB"):
    ACQ_ROWS[_a + "-128"] = (128, dict(acq=ACQ[_a]), ("fused", "none", "mean_argmax", _a, 0, 0))
    ACQ_ROWS[_a + "-130"] = (130, dict(acq=ACQ[_a]), ("all_draws", "none", "mean_argmax", _a, 0, 0))
ACQ_ROWS.update({
    "EI-fant": (130, dict(S=ACQ_S), ("per_fantasy", "none", "mean_argmax", "EI", 0, ACQ_S)),
    "MES": (130, dict(acq=ACQ["MES"], mesK=ACQ_K), ("all_draws", "mes", "mean_argmax", "EI", 1, 0)),
    "MES-fant": (130, dict(acq=ACQ["MES"], mesK=ACQ_K, S=ACQ_S, mes_fantasies=1), ("mes_fant_means", "mes_fant", "mean_argmax", "EI", 0, ACQ_S)),
    "EHVI": (130, dict(acq=ACQ["EHVI"], nmodels=2), ("all_draws", "ehvi", "mean_argmax", "EI", 1, 0)),
    "TS": (130, dict(rhs=RHS["ts"], ts_S=ACQ_S), ("ts", "none", "ts_argmin", "EI", 0, ACQ_S)),
    "KG-pairs": (130, dict(acq=ACQ["KG"], A=ACQ_A), ("kg_pairs", "none", "mean_argmax", "EI", 0, 1 + ACQ_A)),
    "KG-scan": (130, dict(acq=ACQ["KG"], A=ACQ_A, kg_scan=1), ("kg_scan", "none", "mean_argmax", "EI", 0, 1 + ACQ_A)),
    "KG-fant": (130, dict(acq=ACQ["KG"], A=ACQ_A, S=ACQ_S, kg_fantasies=1), ("kgf_lines8", "kgf_value", "mean_argmax", "EI", 0, ACQ_S + ACQ_A)),
    "KG-fant-wide": (130, dict(acq=ACQ["KG"], A=ACQ_A, S=ACQ_S, kg_fantasies=2, kg_scan=1),
                     ("kgf_lines16", "kgw_value", "mean_argmax", "EI", 0, ACQ_S + ACQ_A)),
    "KG-fant-wide-noscan": (130, dict(acq=ACQ["KG"], A=ACQ_A, S=ACQ_S, kg_fantasies=2, kg_scan=0),
                            ("kgf_lines16", "kgw_value", "mean_argmax", "EI", 0, ACQ_S + ACQ_A)),
})


def acq_case(name, **kw):
    """The plan_client case of row NAME at M = 1000, H = 3, D = 2 through the 1 MiB staging buffer (two chunks of one draw per item
    at N = 130) with the 64 MiB floor of the right-hand sides' budget; kw overrides."""
    N, kv, _ = ACQ_ROWS[name]
    return ("ei", dict(dict(kv, N=N, M=1000, H=3, D=2, kstar_budget_bytes=1 << 20, fant_budget=64 << 20), **kw))


def compiler():
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def client(name="plan_client"):
    """Path of the built client tests/c/NAME.cpp (built once per process, into a temporary directory), or None without a
    compiler.  plan_client is over csrc/spx_plan.h; held_client over csrc/spx_held.h (tests/test_held.py); shards_client over
    csrc/spx_shards.h (tests/test_shards.py)."""
    if name not in _clients:
        cxx = compiler()
        if not cxx:
            _clients[name] = None
        else:
            exe = os.path.join(tempfile.mkdtemp(prefix="spx_%s_" % name), name)
            subprocess.check_call([cxx] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "c", name + ".cpp")])
            _clients[name] = exe
    return _clients[name]


def ask(name, text):
    """The output lines of one run of client NAME over the input lines `text`."""
    return subprocess.run([client(name)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()


def plans(cases):
    """One dict of plan fields per case, in order (one run of the client)."""
    text = "".join(kind + "".join(" %s=%d" % (k, int(v)) for k, v in kv.items()) + "\n" for kind, kv in cases)
    res = [json.loads(line) for line in ask("plan_client", text)]
    assert len(res) == len(cases)
    return res


def plan(kind, **kv):
    return plans([(kind, kv)])[0]
