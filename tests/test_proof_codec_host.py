"""cap_amd/csrc/proof_codec.hpp is host+device: this CPU test compiles its CAP_HD decode and encode rule for the host
(tests/cpp/proof_codec_check.cpp) and runs it against params.hpp's g1_decompress_host plus the bound on Fr - the pieces of
capgpu_proof_deserialize - field by field, for records at byte offsets 0..7 with strides 769 and 776; encode then decode is
the identity and gives serialize_g1 / serialize_fr's bytes; every row of the corruption table (length prefixes, the tag,
both flags / infinity with x != 0 / x = p / x = 4 at each of the 13 points, r at each of the 10 scalars, two at once) names
its offset and decodes to all-ones words.  (`-m "not gpu"`)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _run(tmp_path, cxx, flags):
    exe = str(tmp_path / "proof_codec_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-x", "c++"] + flags +
                          [os.path.join(HERE, "cpp", "proof_codec_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad=0" in out.stdout, out.stdout[-800:] + out.stderr[-800:]


def test_codec_against_the_host_reader(tmp_path):
    cxx = next((c for c in ("g++", CLANG, "clang++") if shutil.which(c) or os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    _run(tmp_path, cxx, [])


def test_codec_against_the_host_reader_under_ubsan_and_asan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ for the sanitizer build")
    _run(tmp_path, CLANG, ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"])
