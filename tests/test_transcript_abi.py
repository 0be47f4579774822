"""capgpu_plonk_set_transcript and its companions (include/capgpu.h): declared, exported, bound in Python and Rust, and -
being process-wide switches - usable before capgpu_init.  (`-m "not gpu"`)"""
import ctypes
import os
import re

from cap_amd import lib as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capgpu_plonk_set_transcript", "capgpu_plonk_get_transcript", "capgpu_plonk_sync_stats",
           "capgpu_keccak256_batch_dev")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_are_declared_exported_and_bound():
    header, rust, py = read("include", "capgpu.h"), read("bindings", "capgpu-sys", "src", "lib.rs"), read("cap_amd", "lib.py")
    L = cg.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared in capgpu.h"
        assert hasattr(L, name), name + " is not exported by libcapgpu.so"
        assert "pub fn %s(" % name in rust, name + " is missing from lib.rs"
        assert "load().%s(" % name in py, name + " is not called from lib.py"
    for fn in ("plonk_set_transcript", "plonk_get_transcript", "plonk_sync_stats", "keccak256_batch_dev"):
        assert callable(getattr(cg, fn))


def test_mode_constants_equal_the_headers():
    header = read("include", "capgpu.h")
    host = int(re.search(r"#define CAPGPU_TRANSCRIPT_HOST (\d+)", header).group(1))
    dev = int(re.search(r"#define CAPGPU_TRANSCRIPT_DEVICE (\d+)", header).group(1))
    assert (cg.TRANSCRIPT_HOST, cg.TRANSCRIPT_DEVICE) == (host, dev) == (0, 1)
    rust = read("bindings", "capgpu-sys", "src", "lib.rs")
    assert "CAPGPU_TRANSCRIPT_HOST: c_int = %d" % host in rust and "CAPGPU_TRANSCRIPT_DEVICE: c_int = %d" % dev in rust


def test_set_and_get_round_trip_without_a_device():
    L = cg.load()
    before = cg.plonk_get_transcript()
    try:
        for mode in (cg.TRANSCRIPT_DEVICE, cg.TRANSCRIPT_HOST, "device", "host"):
            cg.plonk_set_transcript(mode)
            want = mode if isinstance(mode, int) else {"host": 0, "device": 1}[mode]
            assert cg.plonk_get_transcript() == want
        for bad in (-1, 2, 77):
            assert L.capgpu_plonk_set_transcript(ctypes.c_int(bad)) == -1      # CAPGPU_ERR_INVALID_ARG
            assert b"capgpu_plonk_set_transcript" in L.capgpu_last_error()
            assert cg.plonk_get_transcript() == 0, "a refused mode changes nothing"
        assert L.capgpu_plonk_get_transcript(None) == -1
    finally:
        cg.plonk_set_transcript(before)
    calls, waits = cg.plonk_sync_stats()
    assert calls >= 0 and waits >= 0
    assert L.capgpu_plonk_sync_stats(None, None) == 0


def test_the_hash_entry_point_refuses_what_it_cannot_do():
    """Without a device: not initialised, loudly.  With one: a negative count and decreasing offsets are refused."""
    from tests import helpers as H
    L = cg.load()
    offs = (ctypes.c_uint64 * 2)(0, 0)
    out = (ctypes.c_uint8 * 32)()
    if not H.gpu_present():
        assert L.capgpu_keccak256_batch_dev(None, offs, 1, out) == -6
        assert b"not initialised" in L.capgpu_last_error()
        return
    cg.init(0)
    assert L.capgpu_keccak256_batch_dev(None, offs, -1, out) == -1          # CAPGPU_ERR_INVALID_ARG
    assert b"capgpu_keccak256_batch_dev" in L.capgpu_last_error()
    bad = (ctypes.c_uint64 * 2)(8, 0)
    assert L.capgpu_keccak256_batch_dev(None, bad, 1, out) == -1
    assert L.capgpu_keccak256_batch_dev(None, offs, 1, out) == 0 and bytes(out).hex().startswith("c5d24601")
