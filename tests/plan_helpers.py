"""Shared by tests/test_plan.py (CPU) and tests/test_gpu_r_plan_runs.py: builds tests/c/plan_client.cpp -- a stand-alone host
program over csrc/spx_plan.h alone -- with the host C++ compiler and the address / undefined-behaviour sanitizers, and asks it
for plans.  A case is ("factor" | "ei", {key: value}); keys are the shape's (plan_client.cpp) and option names."""
import json
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
_client = []


def compiler():
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def client():
    """Path of the built client (built once per process, into a temporary directory), or None without a compiler."""
    if not _client:
        cxx = compiler()
        if not cxx:
            _client.append(None)
        else:
            exe = os.path.join(tempfile.mkdtemp(prefix="spx_plan_"), "plan_client")
            subprocess.check_call([cxx] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "c", "plan_client.cpp")])
            _client.append(exe)
    return _client[0]


def plans(cases):
    """One dict of plan fields per case, in order (one run of the client)."""
    text = "".join(kind + "".join(" %s=%d" % (k, int(v)) for k, v in kv.items()) + "\n" for kind, kv in cases)
    out = subprocess.run([client()], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
    res = [json.loads(line) for line in out.splitlines()]
    assert len(res) == len(cases)
    return res


def plan(kind, **kv):
    return plans([(kind, kv)])[0]
