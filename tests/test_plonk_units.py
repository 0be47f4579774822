"""The prover's translation units ("The prover's units"): plonk.hip holds every kernel and every launch of the
prover; the host-only units - plonk_keys.hip, plonk_solver.hip - hold no device code and reach plonk.hip through prover.hpp.
Two checks that need no GPU: the whole C boundary survived the split - every function include/capgpu.h declares resolves
in the built library - and the rule that keeps a host unit free of device code holds in its text and in everything it
includes.  Both shared headers compile included first in a file that holds nothing else.
(`-m "not gpu"`)"""
import os
import re
import subprocess

import pytest

from cap_amd import lib as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cap_amd", "csrc")
HOST_UNITS = ("plonk_keys.hip", "plonk_solver.hip")
# what only plonk.hip may include: the prover's kernels, the device transcript, and the engine that launches them
DEVICE_HEADERS = ("plonk_kernels.hpp", "check_kernels.hpp", "compact_kernels.hpp", "vars_kernels.hpp", "notes_kernels.hpp",
                  "solve_kernels.hpp", "solve_defer_kernels.hpp", "transcript_dev.hpp", "prove_run.hpp")
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _declared_functions():
    hdr = open(os.path.join(ROOT, "include", "capgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    # a declaration at file scope: return type, name, '(' - a statement that starts a line and is no typedef
    names = re.findall(r"^(?!typedef)[A-Za-z_][\w \t\*]*?\b(capgpu_\w+)\s*\(", hdr, flags=re.M)
    return sorted(set(names))


def _includes(name, seen=None):
    """every header of cap_amd/csrc that `name` includes, directly or through what it includes"""
    seen = set() if seen is None else seen
    for inc in INCLUDE.findall(open(os.path.join(CSRC, name)).read()):
        inc = os.path.normpath(inc)
        if inc in seen or not os.path.exists(os.path.join(CSRC, inc)):
            continue
        seen.add(inc)
        _includes(inc, seen)
    return seen


def test_every_declared_function_is_exported():
    names = _declared_functions()
    assert len(names) > 150, len(names)  # the header declares far more than the dozen names the *_abi tests know
    for probe in ("capgpu_init", "capgpu_plonk_prove_notes_async", "capgpu_plonk_key_deserialize", "capgpu_keccak256_batch_dev",
                  "capgpu_plonk_key_set_solve_form", "capgpu_plonk_graph_stats"):
        assert probe in names, probe  # the parse sees every family
    L = cg.load()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_host_units_hold_no_device_code():
    for unit in HOST_UNITS:
        text = open(os.path.join(CSRC, unit)).read()
        assert "__global__" not in text, unit
        # a call of launch.hpp's launch(), not a name that ends in it (solve_launch_packed, pub_inputs_launch)
        assert not re.search(r"(?<![\w])launch\s*\(", text), unit
        direct = [os.path.basename(i) for i in INCLUDE.findall(text)]
        assert not set(direct) & set(DEVICE_HEADERS), (unit, sorted(set(direct) & set(DEVICE_HEADERS)))
        assert "prover.hpp" in direct, unit  # the door they go through
        reached = {os.path.basename(i) for i in _includes(unit)}  # ... nor through a header that pulls one in
        assert not reached & set(DEVICE_HEADERS), (unit, sorted(reached & set(DEVICE_HEADERS)))


def test_prover_hpp_reaches_no_kernel_header():
    reached = {os.path.basename(i) for i in _includes("prover.hpp")}
    assert "context.hpp" in reached  # the walk follows includes
    assert not reached & set(DEVICE_HEADERS), sorted(reached & set(DEVICE_HEADERS))
    assert not [h for h in reached if h.endswith("_kernels.hpp")], sorted(reached)
    # ... and so does the other header the host units share
    reached = {os.path.basename(i) for i in _includes("plonk_key.hpp")}
    assert not reached & set(DEVICE_HEADERS) and not [h for h in reached if h.endswith("_kernels.hpp")], sorted(reached)


def test_sched_macro_is_plonk_hips_own():
    """CAP_FL_SCHED is set at the top of plonk.hip and by no host unit or shared header of the prover"""
    assert re.search(r"^#define CAP_FL_SCHED 1$", open(os.path.join(CSRC, "plonk.hip")).read(), flags=re.M)
    for name in HOST_UNITS + ("prover.hpp", "plonk_key.hpp"):
        assert "#define CAP_FL_SCHED" not in open(os.path.join(CSRC, name)).read(), name


@pytest.mark.parametrize("header", ["prover.hpp", "plonk_key.hpp"])
def test_shared_header_compiles_alone(header, tmp_path):
    """included first in a file that includes nothing else (host pass of the product's compiler, syntax only)"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC \?= (\S+)", mk, flags=re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)", mk, flags=re.M).group(1)
    src = tmp_path / "alone.hip"
    src.write_text('#include "%s"\n' % header)
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=" + arch, "--cuda-host-only", "-fsyntax-only", "-I", CSRC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
