"""The launch plans' edge pass (csrc/plan_edges.h: plain C++, no HIP) on the CPU: tests/plan_edges/edges_check.cpp --
one hand-written op list per rule with the exact compiled counts, and a seeded random check that the compiled list's
happens-before relation over launches / all-reduces / callouts equals the recorded list's (three replays unrolled) --
built as a stand-alone program with AddressSanitizer + UndefinedBehaviorSanitizer and run."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "plan_edges", "edges_check.cpp")
INC = os.path.join(REPO, "stablediffusion-pytorch_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("plan_edges") / "edges_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", out])
    return out


def test_edge_pass_rules_and_relation(program):
    r = subprocess.run([program, "3000"], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "3000 random lists" in r.stdout and " 0 with a different relation" in r.stdout
    assert r.stdout.rstrip().endswith("ok")


def test_edge_pass_relation_second_seed(program):
    r = subprocess.run([program, "2000", "97"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
