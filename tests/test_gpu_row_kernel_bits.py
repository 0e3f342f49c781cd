"""K7 (als_fold_in), K11 (als_explain) and K13 (als_nnls_rows) return the recorded bits.

The three kernels build their per-row normal equations with the code of csrc/row_system.h,
and every output of theirs is order-fixed by construction.  tests/golden/row_kernel_bits.npz
holds the outputs of a small grid of cases (tools/record_row_kernel_bits.py: ranks 1, 16, 17,
33, 100 and 128, explicit and implicit, rows at the batch-of-32 edges, a repeated item, unknown
items, r <= 0, target counts 0 / 1 / 16 / 17, K13 with and without chunked rows, and one
failing pivot), recorded from the commit the file names.  Each case runs with the sources
stored tight and stored padded with NaN in the padding; both must return the one recorded set.
The inputs are rebuilt from the recorder's seeds and every array must match byte for byte: a
change that moves a bit of these kernels is either a bug or re-records the file.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from als_mi355x import engine as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_row_kernel_bits", os.path.join(ROOT, "tools", "record_row_kernel_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
RUNS = [(*c, wide) for c in REC.cases() for wide in REC.storages(c[0])]
IDS = [f"{c[0]}-{'wide' if c[3] else 'tight'}" for c in RUNS]


@pytest.fixture(scope="module")
def golden():
    with np.load(REC.GOLDEN) as z:
        return {name: z[name] for name in z.files}


def test_fixture_covers_exactly_the_cases(golden):
    assert {n.split("/")[0] for n in golden} == {c[0] for c in REC.cases()} | {"meta"}
    assert os.path.getsize(REC.GOLDEN) < 200 * 1024


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_bits_match_the_recording(run, golden):
    cid, wide = run[0], run[3]
    commit = str(golden["meta/commit"])
    sha, got = REC.run_case(E, torch, *run)
    want = {n.split("/", 1)[1]: a for n, a in golden.items() if n.startswith(cid + "/")}
    assert sha == str(want.pop("inputs_sha256_wide" if wide else "inputs_sha256_tight")), (
        f"case {cid}: the inputs rebuilt from the seeds differ from those recorded at {commit}")
    want.pop("inputs_sha256_tight" if wide else "inputs_sha256_wide", None)
    assert set(got) == set(want), f"case {cid}: arrays {sorted(set(got) ^ set(want))}"
    for name in sorted(want):
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (
            f"case {cid}, {name}: {g.dtype}{g.shape} against {w.dtype}{w.shape} at {commit}")
        # bytes: NaN and -0 count too
        diff = int((g.reshape(-1, 1).view(np.uint8) != w.reshape(-1, 1).view(np.uint8)).any(1).sum())
        assert diff == 0, (f"case {cid}, {name}: {diff} of {g.size} values differ from the bits "
                           f"recorded at commit {commit}")
    if cid == "pivot":  # the recording is of a failure: row 1 reported, its outputs zeroed
        assert int(got["k7_status"][0]) == 2 and int(got["k11_status"][0]) == 2
        assert not got["k7_X"][1].any() and not got["k11_score"][2:].any()
