"""The asynchronous entry points of include/capgpu.h (tickets, capgpu_plonk_reserve, the allocator and ticket counters): each
is exported by the library, declared in the header and bound in the Rust shim, and - like every compute entry point - has
no host path: before capgpu_init it refuses.  (`-m "not gpu"`)"""
import os
import re
import subprocess
import sys

from cap_amd import lib as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capgpu_plonk_prove_batch_async", "capgpu_plonk_prove_multi_async", "capgpu_wait", "capgpu_async_stats",
       "capgpu_plonk_reserve", "capgpu_scratch_stats")


def test_new_symbols_are_exported_declared_and_bound():
    L = cg.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "capgpu.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "capgpu-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(L, name), f"{name} is not exported by libcapgpu.so"
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/capgpu.h"
        assert re.search(rf"pub fn {name}\s*\(", rs), f"{name} is not bound in bindings/capgpu-sys/src/lib.rs"
    assert re.search(r"#define CAPGPU_ERR_BUSY \(-10\)", hdr) and "pub const CAPGPU_ERR_BUSY: c_int = -10;" in rs
    assert cg.ERR_BUSY == -10
    for name in ("plonk_prove_batch_async", "plonk_prove_multi_async", "plonk_reserve", "scratch_stats", "async_stats", "Ticket"):
        assert hasattr(cg, name)
    hpp = open(os.path.join(ROOT, "include", "capgpu_proof.hpp")).read()
    assert "prove_batch_async" in hpp and "capgpu_wait" in hpp


# a process that never called capgpu_init (this one may have, on a machine with a GPU: the suite shares a session)
CHILD = r"""
import ctypes
from cap_amd import lib as cg
L = cg.load()
u64, sz, i32 = ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
buf = (ctypes.c_uint64 * 64)()
proofs = (cg.Proof * 1)()
t, done = u64(0), i32(0)
a, b, m, ms = u64(0), u64(0), ctypes.c_uint32(0), ctypes.c_double(0)
handles = (ctypes.c_uint64 * 1)(1)
codes = {
    "batch_async": L.capgpu_plonk_prove_batch_async(u64(1), 1, buf, buf, sz(1), None, sz(0), buf, 0, proofs, ctypes.byref(t)),
    "multi_async": L.capgpu_plonk_prove_multi_async(handles, 1, buf, buf, sz(1), None, None, buf, 0, proofs, ctypes.byref(t)),
    "empty_batch": L.capgpu_plonk_prove_batch_async(u64(1), 0, None, None, sz(0), None, sz(0), None, 0, None, ctypes.byref(t)),
    "wait": L.capgpu_wait(u64(5), ctypes.c_uint32(0), ctypes.byref(done)),
    "async_stats": L.capgpu_async_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(m)),
    "reserve": L.capgpu_plonk_reserve(u64(1), 8, 0, -1),
    "scratch_stats": L.capgpu_scratch_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(ms)),
}
msg = L.capgpu_last_error().decode()
print(sorted(codes.items()), "|", t.value, done.value, "|", msg)
"""


def test_no_host_path_before_init():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    out = r.stdout.strip().splitlines()[-1]
    codes = dict(eval(out.split("|")[0]))
    for name, rc in codes.items():
        # (an unknown ticket may also be answered CAPGPU_ERR_BAD_HANDLE; here the library is not initialised at all)
        assert rc == -6 or (name == "wait" and rc == -4), (name, rc, out)
    assert out.split("|")[1].split() == ["0", "0"], "no ticket was handed out, nothing was reported done"
    assert "not initialised" in out.split("|")[2]
