"""The grouped GEMM planner's carry mode (mkgp::plan_carry, macaw_llm_amd/csrc/gemm_group_plan.h) on the CPU:
tests/gemm_group_carry_main.cpp is a stand-alone program that includes the planner header.  Built with the host compiler and run
twice -- plainly, and with -fsanitize=address,undefined.  It checks
  * the plan's shape in carry mode: the taken tiles are a prefix of the queue, the runs cover them, and after a final flush every
    tile of every problem was computed exactly once
  * least idle: 800 seeded random launches at 8 planned CUs with at least gaps + 2 n t_max queued; the planner's priced idle time
    equals the least that a brute force over the filler counts per class of main cost finds for levels in [lmain, lmain + t_max)
    (fillers of one K), or exceeds it by less than one t_max (mixed K); 400 launches with too little queued plan as balance mode
  * 32 cfg-3 decoder layers with one carried queue and a final flush against the same layers drained per layer, summing the
    priced heaviest workgroup over all launches: at most 0.975 of today's at 256 planned CUs (1874.0 / 1934.1 = 0.969 per layer
    in steady state), not longer at 248 and 240; never more than MAX_FILL live problems, never a launch short of fillers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gemm_group_carry_main.cpp")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan+ubsan"])
def test_the_carry_program_passes(tmp_path, flags):
    r = subprocess.run([_build(tmp_path, "carry", flags)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-1].startswith("OK "), r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[-1]) > 3000         # launches planned and checked


def test_the_cfg3_sequence_at_256_cus_settles_at_the_least_idle_levels(tmp_path):
    """a steady-state layer (the tenth): idle 48 + 1384 + 256 + 1204 K-tile units in its four launches, all it queued is taken
    (3088 tiles), and the backlog behind it stays within half a round of one tile per workgroup"""
    r = subprocess.run([_build(tmp_path, "carry", []), "dump", "256"], capture_output=True, text=True, check=True)
    lines = [ln for ln in r.stdout.split("\n") if " carry layer " in ln]
    layer = [ln for ln in lines if " layer 10 " in ln]
    assert [int(ln.split("idle ")[1].split()[0]) for ln in layer] == [48, 1384, 256, 1204], layer
    left = [int(ln.split("left ")[1].split(",")[0]) for ln in lines if ln.split(":")[0].endswith("launch 4")]
    assert all(128 <= x <= 384 for x in left), left
    took = sum(int(ln.split("took ")[1].split(",")[0]) for ln in lines)
    assert took == 32 * (688 + 1376 + 256 + 768)
