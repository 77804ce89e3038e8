"""The work plan of a grouped GEMM launch (macaw_llm_amd/csrc/gemm_group_plan.h) on the CPU: tests/gemm_group_plan_main.cpp is a
stand-alone program that includes the planner header.  Built with the host compiler and run twice -- plainly, and with
-fsanitize=address,undefined.  It checks, for the backward of one cfg-3 decoder layer (774 x 64 with 688 x 72 queued, 288 x 344
with + 1376 x 72, 288 x 64 with + 256 x 72, 288 x 192 with + 768 x 72 and drain) at 256 and at 240 planned CUs, and for 800 seeded
random queues at 8 planned CUs (400 with one K for all fillers, 400 with mixed K):
  * every tile of every problem is assigned exactly once over the launches
  * heaviest - lightest workgroup <= one filler tile's cost whenever enough fillers are queued
  * drain leaves nothing; a balancing launch leaves the rest queued and never lengthens the launch by more than half a tile
  * workgroups without work, empty launches, whole-round main problems and filler-only launches are legal."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gemm_group_plan_main.cpp")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan+ubsan"])
def test_the_planner_program_passes(tmp_path, flags):
    r = subprocess.run([_build(tmp_path, "plan", flags)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 1500          # launches planned and checked


def test_the_cfg3_sequence_at_256_cus_takes_what_the_rule_says(tmp_path):
    """dx(down): 250 workgroups are one 64-K-tile main tile short and take one 72-K-tile filler tile each; dx(gate|up): 224 are one
    344-K-tile tile short = 4.45 filler tiles -> 4 each; dx(o): 224 x 1; the draining dx(q|k|v) launch takes the remaining 1718."""
    r = subprocess.run([_build(tmp_path, "plan", []), "dump", "256"], capture_output=True, text=True, check=True)
    took = [int(line.split("took ")[1].split(",")[0]) for line in r.stdout.strip().split("\n")]
    assert took == [250, 896, 224, 1718] and sum(took) == 688 + 1376 + 256 + 768
