"""The device conformance check on the MI355X: the op table of tests/hip/devcheck_ops.hpp - field29.hpp, field.hpp,
curve29.hpp (term_mul included), quad29.hpp on real lanes (QuadDev, full waves of 16 quads with mixed cases and a partial
last wave) and pairing29.hpp - in gfx950 kernels built with the product's flags, one vector per lane, against Python
integers and the oracle (tests/devcheck_vectors.py), and limb for limb against the host driver's result file.

The device binary (tests/hip/devcheck, built by build()) runs ONCE, as one fresh child process under its own time limit;
the tests only parse its result file, one test per group.  Measured on the MI355X: 0.72 s of wall time for the whole
binary, 65 441 records (MEASURED_S below), 15 s for this module with the host driver's build and the Python checks; the limit is five times that, not below 60 s - the margin is for a busy shared machine.

Exceptions to the limb-for-limb comparison with the host: none.  The CPU experiment (tests/test_devcheck_host.py: g++
against clang++, -O1 against -O2, 64- against 32-bit limbs in field.hpp, schedule 0 against 1) shows the un-reduced
representatives to be determined by the source, so every op is compared limb for limb."""
import os
import subprocess
import time

import pytest

from tests import devcheck_vectors as dv
from tests.devcheck_vectors import build_host, run_driver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "hip", "devcheck")
SOURCES = [os.path.join(HERE, "hip", n) for n in ("devcheck.hip", "devcheck_ops.hpp", "devcheck_io.hpp")] + \
    [os.path.join(dv.ROOT, "cap_amd", "csrc", n) for n in ("field.hpp", "field29.hpp", "curve29.hpp", "quad29.hpp",
                                                             "pairing29.hpp", "pairing.hpp", "curve.hpp")]
MEASURED_S = 0.72
TIME_LIMIT_S = max(60.0, 5 * MEASURED_S)


def _binary():
    """the binary build() made; rebuilt with hipcc only if it is missing or older than its sources; a failure otherwise"""
    fresh = os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(s) for s in SOURCES)
    if not fresh:
        assert os.path.exists("/opt/rocm/bin/hipcc"), "tests/hip/devcheck is missing or stale and there is no hipcc"
        subprocess.check_call(["make", "-C", os.path.join(dv.ROOT, "cap_amd", "csrc"), "../../tests/hip/devcheck"])
    return EXE


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("devcheck_gpu")
    recs, g2 = dv.generate()
    vec = str(d / "vectors.bin")
    dv.write_vectors(vec, recs, g2)
    assert dv.host_cxx(), "no host C++ compiler for the host driver"
    host = run_driver(build_host(str(d / "devcheck_host"), ["-O1"]), vec, str(d / "host.bin"))
    exe, res = _binary(), str(d / "device.bin")
    t0 = time.time()
    try:
        out = subprocess.run([exe, vec, res], capture_output=True, text=True, timeout=TIME_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the device binary did not finish within {TIME_LIMIT_S} s: {(e.stderr or b'')[-800:]}")
    wall = time.time() - t0
    print(f"devcheck: device binary wall time {wall:.2f} s")
    assert out.returncode == 0, f"the device binary ended with {out.returncode}: {out.stderr[-1200:]}"
    return {"recs": recs, "dev": dv.read_results(res), "host": host, "wall": wall}


@pytest.mark.parametrize("group", dv.GROUPS)
def test_device_matches_python_and_the_host_limb_for_limb(run, group):
    fails, counts = dv.check_group(group, run["recs"][group], run["dev"][group])
    assert not fails, f"{group} on the device:\n" + dv.format_fails(fails)
    floors = dv.check_floors(group, run["recs"][group], counts)
    assert not floors, "\n".join(floors)
    diff = dv.compare_files(run["dev"], run["host"], [group])
    assert not diff, f"{group}: {len(diff)} records differ from the host driver's limbs, first: " + \
        "; ".join(run["recs"][g][i].describe() for g, i in diff[:5])
