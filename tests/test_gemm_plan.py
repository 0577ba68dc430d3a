"""The GEMM launch policy (csrc/gemm_plan.h: tile, waves, split, grid per problem) against the
table recorded at the launch sites of the code it was factored out of (tests/golden/gemm_plans.tsv:
the step's shapes, the shapes of tests/test_gpu_gemm.py, a row on either side of every threshold
and the non-default knob sets).  The header has no HIP in it, so the plain host compiler builds the
dump program; a policy change shows up here as a diff of that table."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN, N_OUT = 29, 16


def test_gemm_plans_match_recorded_table(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++ / g++ / clang++) on PATH"
    exe = str(tmp_path / "gemm_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "gemm_plan_dump.cpp"),
                    "-o", exe], check=True)
    table = os.path.join(ROOT, "tests", "golden", "gemm_plans.tsv")
    with open(table) as f:
        lines = [ln.rstrip("\n") for ln in f]
    names = lines[[i for i, ln in enumerate(lines) if ln.startswith("#")][-1]][2:].split("\t")
    cases = [ln.split("\t") for ln in lines if ln and not ln.startswith("#")]
    assert len(names) == N_IN + N_OUT and len(cases) > 400 and all(len(c) == N_IN + N_OUT for c in cases)
    out = subprocess.run([exe, table], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    bad = []
    for case, got in zip(cases, out):
        want, got = case[N_IN:], got.split("\t")
        diff = [f"{n}: {g} != {w}" for n, g, w in zip(names[N_IN:], got, want) if g != w]
        if len(got) != N_OUT or diff:
            bad.append(" ".join(f"{n}={v}" for n, v in zip(names, case[:N_IN])) + " -> " + ", ".join(diff))
    assert not bad, f"{len(bad)} of {len(cases)} plans differ:\n" + "\n".join(bad[:20])
