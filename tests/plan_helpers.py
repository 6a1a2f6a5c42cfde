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
