"""csrc/task_order.h on the host: tests/task_order_main.cpp (its own main) built with the
host compiler and run.  It checks that task t -> (chunk | light position) is a bijection
(exhaustively for (n_chunks, n_light) in [0, 48]^2 and at the bench shapes, sampled at
n_chunks + n_light = 2^31 - 1), that each list keeps its order, that list A is spread
evenly and that the merged lists run out within one task of each other."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "recommender-system-using-apache-spark-mllib-_amd", "csrc")


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/bin/hipcc"):
        if c and shutil.which(c):
            return c
    raise AssertionError("no C++ compiler found")


# the shipped parameters, then others the sweep used: no tail, f = 0 (chunks only), large f
@pytest.mark.parametrize("defs", [(), ("-DALS_TASK_TAIL_DEN=0",),
                                  ("-DALS_TASK_SPLIT_NUM=0", "-DALS_TASK_SPLIT_DEN=1"),
                                  ("-DALS_TASK_SPLIT_NUM=1", "-DALS_TASK_SPLIT_DEN=2",
                                   "-DALS_TASK_TAIL_DEN=0")])
def test_task_order_host_program(tmp_path, defs):
    exe = str(tmp_path / "task_order_check")
    subprocess.check_call([_cxx(), "-O2", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", *defs, "-I", CSRC,
                           os.path.join(HERE, "task_order_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "task order ok" in p.stdout
