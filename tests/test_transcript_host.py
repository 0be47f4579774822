"""cap_amd/csrc/transcript_dev.hpp is host+device: this CPU test compiles its CAP_HD parts for the host under
-fsanitize=undefined and runs them (tests/cpp/transcript_dev_check.cpp) against keccak.hpp and host_util.hpp - the lane
form of Keccak-f on 64 simulated lanes, sponge framing and padding at every length 0..272, the fork, chained challenges,
the 48-byte reduction, the variable-time inversion, point compression at its boundaries and the linearisation scalars
both transcript modes share.  (`-m "not gpu"`)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _build(tmp_path, cxx, flags):
    exe = str(tmp_path / "transcript_dev_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17"] + flags + [os.path.join(HERE, "cpp", "transcript_dev_check.cpp"), "-o", exe])
    return exe


def test_transcript_parts_against_the_host_transcript_under_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    exe = _build(tmp_path, CLANG, ["-fsanitize=undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]


def test_transcript_parts_with_the_32_bit_host_multiplication(tmp_path):
    """CAP_HOST_MUL32: the host runs the 32-bit-limb multiplication and the Fermat inversion the device runs"""
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = _build(tmp_path, cxx, ["-DCAP_HOST_MUL32"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]
