"""The headers that csrc/gram_solve.hip is made of are self-contained: a translation unit that
holds nothing but the #include of one of them compiles for gfx950 (syntax only), so each header
includes what it uses and none leans on the order in which gram_solve.hip includes them.
gram_solve.hip must include every header of the list, directly or through another, which keeps
the list from going stale.  CPU only: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recommender-system-using-apache-spark-mllib-_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

HEADERS = ["solve_config.h", "gram_accumulate.h", "solve_guards.h", "panel_solve.h", "w1_solve.h",
           "partial_slots.h", "dual_solve.h", "rescue64.h", "yty.h"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _includes(name, seen):
    """Quoted includes of csrc/<name>, transitively (files of csrc only)."""
    for inc in re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M):
        if inc not in seen and "/" not in inc and os.path.exists(os.path.join(CSRC, inc)):
            seen.add(inc)
            _includes(inc, seen)
    return seen


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    tu = tmp_path / "tu.hip"
    tu.write_text(f'#include "{header}"\n')
    p = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-I", CSRC,
                        str(tu)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]


def test_gram_solve_includes_every_header():
    reached = _includes("gram_solve.hip", set())
    assert not [h for h in HEADERS if h not in reached]
    # and the list names every solve header there is: the other headers of csrc are shared
    # with other translation units and were there before the split
    others = {"als_common.h", "task_order.h"}
    assert reached - others == set(HEADERS)
