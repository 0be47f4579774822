"""The arithmetic of the NTT kernels and of the lazy-field round kernels on the MI355X, function by function:
tests/hip/elemcheck - built by build() from cap_amd/csrc/ntt_elem29.hpp and round_elem29.hpp with the product's flags -
runs the records of tests/elemcheck_vectors.py, one lane each: the
stage butterflies singly with given twiddle pairs (both twiddle forms, the s == 0 round with its zero shortcuts), the
element steps of the column and row passes in every form of the plans, the bodies of ntt3_combine / ntt3_combine5, and the row and point bodies of k_perm_numden, k_kx_columns, both forms of
k_quotient and k_lincomb.

Asserted: every raw output word - all nine limbs of an fl result - equals the host twin's (tests/cpp/ntt_elem_check.cpp,
bound assertions on), bit for bit.  The device build takes mul_lo32 and mad_wide through inline v_mad_u64_u32 and the host
does not; tests/test_ntt_elem_host.py and tests/test_round_elem_host.py check the host twin against Python integers and the bound table, so this is what
carries those checks over to the compile that runs in the prover.

The binary runs ONCE, as one fresh child process under its own time limit; the tests only parse its result file.
TIME_LIMIT_S is the floor tests/test_gpu_devcheck.py uses for a binary of this kind; MEASURED_S is the binary's wall time
on the MI355X (0.63 s for the 3200 records), below a fifth of the limit."""
import os
import subprocess
import time

import numpy as np
import pytest

from tests import elemcheck_vectors as ev
from tests.test_field29_host import CPP, _cxx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "hip", "elemcheck")
MEASURED_S = 0.63
TIME_LIMIT_S = 60.0


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert os.path.exists(EXE), "tests/hip/elemcheck is missing: build() makes it (make -C cap_amd/csrc)"
    d = tmp_path_factory.mktemp("elemcheck")
    recs = ev.generate()
    inp, host_res, dev_res = str(d / "records.bin"), str(d / "host.bin"), str(d / "device.bin")
    ev.write_records(inp, recs)
    twin = str(d / "ntt_elem_check")
    subprocess.check_call([_cxx(), "-O1", "-std=c++17", os.path.join(CPP, "ntt_elem_check.cpp"), "-o", twin])
    out = subprocess.run([twin, "elem", "0", inp, host_res], capture_output=True, text=True)
    assert out.returncode == 0, f"the host twin ended with {out.returncode}: {out.stderr[-1200:]}"
    t0 = time.time()
    try:
        out = subprocess.run([EXE, inp, dev_res], capture_output=True, text=True, timeout=TIME_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"elemcheck did not finish within {TIME_LIMIT_S} s: {(e.stderr or b'')[-800:]}")
    wall = time.time() - t0
    print(f"elemcheck: {len(recs)} records, wall time {wall:.2f} s")
    assert out.returncode == 0, f"elemcheck ended with {out.returncode}: {out.stderr[-1200:]}"
    return {"recs": recs, "host": ev.read_results(host_res, len(recs)), "dev": ev.read_results(dev_res, len(recs)),
            "wall": wall}


@pytest.mark.parametrize("op", ev.OPS)
def test_device_words_equal_the_host_twins(run, op):
    rows = np.array([i for i, r in enumerate(run["recs"]) if r.op == ev.OPS.index(op)])
    assert len(rows) >= 300
    host, dev = run["host"][rows], run["dev"][rows]
    assert host.any(), "the host twin wrote nothing for this op"
    bad = np.nonzero((host != dev).any(axis=1))[0]
    assert not len(bad), f"{op}: {len(bad)} of {len(rows)} records differ from the host twin's words, first record " \
                         f"{rows[bad[0]]}: host {host[bad[0]].tolist()} device {dev[bad[0]].tolist()}"


def test_the_run_stays_below_a_fifth_of_its_limit(run):
    assert run["wall"] < TIME_LIMIT_S / 5, f"elemcheck took {run['wall']:.2f} s: split the record file"
