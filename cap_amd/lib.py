"""ctypes binding of include/capgpu.h (the drop-in C ABI).  No compute happens in Python."""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("CAPGPU_LIBRARY") or os.path.join(_HERE, "libcapgpu.so")  # override: A/B builds in tools/
_lib = None

NUM_WIRE_TYPES = 5
NUM_SELECTORS = 13

CAPGPU_OK = 0
ERR_NAMES = {
    -1: "CAPGPU_ERR_INVALID_ARG", -2: "CAPGPU_ERR_NO_DEVICE", -3: "CAPGPU_ERR_HIP", -4: "CAPGPU_ERR_BAD_HANDLE",
    -5: "CAPGPU_ERR_OOM", -6: "CAPGPU_ERR_NOT_INITIALISED", -7: "CAPGPU_ERR_PROOF", -8: "CAPGPU_ERR_SERIALIZATION",
    -9: "CAPGPU_ERR_COMM",
}

u64p = ctypes.POINTER(ctypes.c_uint64)


class CapGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class Proof(ctypes.Structure):
    """capgpu_proof (include/capgpu.h) == jf_plonk::proof_system::structs::Proof fields."""
    _fields_ = [
        ("wires_poly_comms", (ctypes.c_uint64 * 8) * NUM_WIRE_TYPES),
        ("prod_perm_poly_comm", ctypes.c_uint64 * 8),
        ("split_quot_poly_comms", (ctypes.c_uint64 * 8) * NUM_WIRE_TYPES),
        ("opening_proof", ctypes.c_uint64 * 8),
        ("shifted_opening_proof", ctypes.c_uint64 * 8),
        ("wires_evals", (ctypes.c_uint64 * 4) * NUM_WIRE_TYPES),
        ("wire_sigma_evals", (ctypes.c_uint64 * 4) * (NUM_WIRE_TYPES - 1)),
        ("perm_next_eval", ctypes.c_uint64 * 4),
    ]


class VerifyingKey(ctypes.Structure):
    _fields_ = [
        ("domain_size", ctypes.c_uint64),
        ("num_inputs", ctypes.c_uint64),
        ("k", (ctypes.c_uint64 * 4) * NUM_WIRE_TYPES),
        ("selector_comms", (ctypes.c_uint64 * 8) * NUM_SELECTORS),
        ("sigma_comms", (ctypes.c_uint64 * 8) * NUM_WIRE_TYPES),
    ]


def lib_path() -> str:
    return _SO


def load():
    """Load libcapgpu.so.  Fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise CapGpuError(-2, f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C cap_amd/csrc).  There is no CPU fallback.")
    L = ctypes.CDLL(_SO)
    L.capgpu_last_error.restype = ctypes.c_char_p
    L.capgpu_version.restype = ctypes.c_char_p
    _lib = L
    return L


def check(rc: int):
    if rc != CAPGPU_OK:
        raise CapGpuError(rc, load().capgpu_last_error().decode())


def init(device: int | None = None, devices=None):
    """One device (`device`; default LOCAL_RANK, the process-per-GPU launch) or, with `devices`, the list of HIP device
    ids this ONE process drives (capgpu_init(device_ids, n): one context per id)."""
    L = load()
    if devices is None:
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        devices = [device]
    ids = (ctypes.c_int * len(devices))(*devices)
    check(L.capgpu_init(ids, len(devices)))
    return L


def shutdown():
    load().capgpu_shutdown()


def device_count() -> int:
    n = ctypes.c_int(0)
    check(load().capgpu_device_count(ctypes.byref(n)))
    return n.value


def physical_device_count() -> int:
    """distinct HIP devices behind the contexts (device_count() counts CONTEXTS: four on one bound GPU by default)"""
    out = ctypes.c_int(0)
    check(load().capgpu_physical_device_count(ctypes.byref(out)))
    return out.value


def timer_begin():
    check(load().capgpu_timer_begin())


def timer_end() -> float:
    """milliseconds of device time on the calling thread's context since timer_begin (HIP events on its stream)"""
    out = ctypes.c_double(0)
    check(load().capgpu_timer_end(ctypes.byref(out)))
    return out.value


def set_stream(stream=None):
    """capgpu_set_stream: the calling thread's context enqueues on the caller's hipStream_t from now on - an int handle or
    anything with a .cuda_stream attribute (torch.cuda.Stream); None restores the library's own stream.  The stream being
    left is drained first."""
    handle = getattr(stream, "cuda_stream", stream)
    check(load().capgpu_set_stream(ctypes.c_void_p(int(handle) if handle else None)))


@contextlib.contextmanager
def on_stream(stream):
    """the body's calls of this thread's context run on `stream` (see set_stream); the library's own stream is restored
    on the way out, exceptions included"""
    set_stream(stream)
    try:
        yield stream
    finally:
        set_stream(None)


def set_device(slot: int):
    """bind the calling thread to context `slot` (-1: unbind)"""
    check(load().capgpu_set_device(int(slot)))


def get_device():
    s, d = ctypes.c_int(0), ctypes.c_int(0)
    check(load().capgpu_get_device(ctypes.byref(s), ctypes.byref(d)))
    return s.value, d.value


def mem_info():
    """(free, total) device memory in bytes"""
    f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_mem_info(ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value


def trim():
    """capgpu_trim: release the scratch, pinned result areas and captured graphs of every idle context.
    Returns (device bytes released, contexts skipped because a call was running on them)."""
    b, busy = ctypes.c_uint64(0), ctypes.c_int(0)
    check(load().capgpu_trim(ctypes.byref(b), ctypes.byref(busy)))
    return b.value, busy.value


def set_memory_limit(scratch_bytes_per_device: int):
    """capgpu_set_memory_limit: cap on the scratch the library holds per device (0 = none); a call that would grow past it
    fails with CAPGPU_ERR_OOM (CapGpuError code -5) after trimming the device's idle contexts."""
    check(load().capgpu_set_memory_limit(ctypes.c_uint64(scratch_bytes_per_device)))


def scratch_info():
    """(scratch bytes held on the calling thread's device, the cap - 0 = none)"""
    b, lim = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_scratch_info(ctypes.byref(b), ctypes.byref(lim)))
    return b.value, lim.value


def trace_enable(on: bool):
    check(load().capgpu_trace_enable(int(bool(on))))


def trace_dump(path: str) -> int:
    n = ctypes.c_uint64(0)
    check(load().capgpu_trace_dump(path.encode(), ctypes.byref(n)))
    return n.value


def _p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u64p)


# ---- device buffers ----------------------------------------------------------------------------
class DevBuf:
    def __init__(self, nbytes: int):
        self.ptr = ctypes.c_void_p()
        self.nbytes = nbytes
        check(load().capgpu_malloc(ctypes.byref(self.ptr), ctypes.c_size_t(nbytes)))

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        check(load().capgpu_memcpy_h2d(b.ptr, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes)))
        return b

    def view(self, offset_bytes: int, nbytes: int) -> "DevBuf":
        """a non-owning window of this buffer (the parent must outlive it)"""
        assert 0 <= offset_bytes and offset_bytes + nbytes <= self.nbytes
        v = DevBuf.__new__(DevBuf)
        v.ptr = ctypes.c_void_p(self.ptr.value + offset_bytes)
        v.nbytes = nbytes
        v._view = True
        return v

    @classmethod
    def from_ptr(cls, ptr: int, nbytes: int) -> "DevBuf":
        """a non-owning buffer over device memory someone else allocated (a torch tensor's data_ptr()): never freed here;
        the owner must outlive it"""
        assert ptr and nbytes >= 0
        v = cls.__new__(cls)
        v.ptr = ctypes.c_void_p(int(ptr))
        v.nbytes = nbytes
        v._view = True
        return v

    def upload(self, a: np.ndarray):
        """overwrite the buffer's first a.nbytes bytes (same device address: resident inputs of a replayed schedule)"""
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        check(load().capgpu_memcpy_h2d(self.ptr, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes)))

    def to_numpy(self, dtype=np.uint64, count: int | None = None, offset_bytes: int = 0) -> np.ndarray:
        itemsize = np.dtype(dtype).itemsize
        n = (self.nbytes - offset_bytes) // itemsize if count is None else count
        out = np.empty(n, dtype=dtype)
        src = ctypes.c_void_p(self.ptr.value + offset_bytes)
        check(load().capgpu_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), src, ctypes.c_size_t(n * itemsize)))
        return out

    def free(self):
        if getattr(self, "_view", False):
            self.ptr = ctypes.c_void_p()
            return
        if self.ptr and self.ptr.value:
            check(load().capgpu_free(self.ptr))
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sync_all():
    """capgpu_sync_all: hipDeviceSynchronize on every bound device"""
    check(load().capgpu_sync_all())


def runtime_info():
    """(HIP runtime version, HIP driver version) the process runs on - the first libamdhip64.so.7 the loader met"""
    r, d = ctypes.c_int(0), ctypes.c_int(0)
    check(load().capgpu_runtime_info(ctypes.byref(r), ctypes.byref(d)))
    return r.value, d.value


def sync():
    check(load().capgpu_sync())


# ---- SRS -----------------------------------------------------------------------------------------
def srs_upload(bases: np.ndarray, montgomery: bool = True) -> int:
    """bases: (n, 8) uint64 packed affine points."""
    bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
    h = ctypes.c_uint64()
    check(load().capgpu_srs_upload(bases.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(bases.shape[0]),
                                   ctypes.c_size_t(64), int(montgomery), ctypes.byref(h)))
    return h.value


def _limbs(v: int):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def srs_generate(tau: int, n: int) -> int:
    h = ctypes.c_uint64()
    check(load().capgpu_srs_generate(_limbs(tau), ctypes.c_size_t(n), ctypes.byref(h)))
    return h.value


def srs_generate_hiding(tau: int, gamma: int, n: int) -> int:
    h = ctypes.c_uint64()
    check(load().capgpu_srs_generate_hiding(_limbs(tau), _limbs(gamma), ctypes.c_size_t(n), ctypes.byref(h)))
    return h.value


def srs_generate_affine_seq(a: int, b: int, n: int) -> int:
    h = ctypes.c_uint64()
    check(load().capgpu_srs_generate_affine_seq(_limbs(a), _limbs(b), ctypes.c_size_t(n), ctypes.byref(h)))
    return h.value


def srs_download(handle: int, offset: int, n: int) -> np.ndarray:
    out = np.empty((n, 8), dtype=np.uint64)
    check(load().capgpu_srs_download(ctypes.c_uint64(handle), ctypes.c_size_t(offset), ctypes.c_size_t(n),
                                     out.ctypes.data_as(ctypes.c_void_p)))
    return out


def srs_free(handle: int):
    check(load().capgpu_srs_free(ctypes.c_uint64(handle)))


def srs_shards(handle: int) -> int:
    n = ctypes.c_int(0)
    check(load().capgpu_srs_shards(ctypes.c_uint64(handle), ctypes.byref(n)))
    return n.value


def srs_size(handle: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().capgpu_srs_size(ctypes.c_uint64(handle), ctypes.byref(n)))
    return n.value


# ---- MSM -----------------------------------------------------------------------------------------
def msm_g1(handle: int, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
    """scalars (n,4) canonical -> Jacobian (12,) Montgomery."""
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(12, dtype=np.uint64)
    check(load().capgpu_msm_g1(ctypes.c_uint64(handle), ctypes.c_size_t(offset), _p(scalars),
                               ctypes.c_size_t(scalars.shape[0]), _p(out)))
    return out


def lagrange_commit(handle: int, log_n: int, scalars_mont: np.ndarray) -> np.ndarray:
    """KZG commitment from VALUES on the 2^log_n domain (+ up to three blinders): MSM on the Lagrange-form commit key"""
    sc = np.ascontiguousarray(scalars_mont, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(12, np.uint64)
    check(load().capgpu_msm_g1_lagrange(ctypes.c_uint64(handle), ctypes.c_uint32(log_n), _p(sc), ctypes.c_size_t(sc.shape[0]),
                                        1, _p(out)))
    return out


def msm_g1_batch(handle: int, scalar_list, offsets=None) -> np.ndarray:
    cnt = len(scalar_list)
    arrs = [np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4) for s in scalar_list]
    offs = (ctypes.c_size_t * cnt)(*([0] * cnt if offsets is None else offsets))
    ns = (ctypes.c_size_t * cnt)(*[a.shape[0] for a in arrs])
    ptrs = (u64p * cnt)(*[_p(a) for a in arrs])
    out = np.zeros((cnt, 12), dtype=np.uint64)
    check(load().capgpu_msm_g1_batch(ctypes.c_uint64(handle), offs, ptrs, ns, cnt, _p(out)))
    return out


def msm_g1_dev(handle: int, d_scalars: DevBuf, n: int, count: int = 1, stride: int | None = None,
               montgomery: bool = False, offset: int = 0, d_out: DevBuf | None = None) -> DevBuf:
    if d_out is None:
        d_out = DevBuf(96 * count)
    check(load().capgpu_msm_g1_dev(ctypes.c_uint64(handle), ctypes.c_size_t(offset), d_scalars.ptr,
                                   ctypes.c_size_t(n if stride is None else stride), ctypes.c_size_t(n), count,
                                   int(montgomery), d_out.ptr))
    return d_out


def msm_scalars_upload(handle: int, scalars: np.ndarray, offset: int = 0) -> int:
    """scalars (count, n, 4) or (n, 4) in host memory -> a scalar set resident with the SRS's point ranges
    (capgpu_msm_scalars_upload: each slice goes to the device that holds its points)."""
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    scalars = scalars.reshape(1, -1, 4) if scalars.ndim == 2 else scalars
    count, n = scalars.shape[0], scalars.shape[1]
    h = ctypes.c_uint64(0)
    check(load().capgpu_msm_scalars_upload(ctypes.c_uint64(handle), ctypes.c_size_t(offset), _p(scalars.reshape(-1)),
                                           ctypes.c_size_t(n), ctypes.c_size_t(n), count, ctypes.byref(h)))
    return h.value


def msm_scalars_scatter_dev(handle: int, d_scalars: DevBuf, n: int, count: int = 1, stride: int | None = None,
                            offset: int = 0) -> int:
    """the same from device memory of the calling thread's context (one peer copy per slice, once)"""
    h = ctypes.c_uint64(0)
    check(load().capgpu_msm_scalars_scatter_dev(ctypes.c_uint64(handle), ctypes.c_size_t(offset), d_scalars.ptr,
                                                ctypes.c_size_t(n if stride is None else stride), ctypes.c_size_t(n),
                                                count, ctypes.byref(h)))
    return h.value


def msm_scalars_free(scalars_handle: int):
    check(load().capgpu_msm_scalars_free(ctypes.c_uint64(scalars_handle)))


def msm_g1_resident(handle: int, scalars_handle: int, count: int = 1, montgomery: bool = False,
                    d_out: DevBuf | None = None) -> DevBuf:
    """MSM(s) on a resident scalar set: only the 96-byte partials move between devices."""
    if d_out is None:
        d_out = DevBuf(96 * count)
    check(load().capgpu_msm_g1_resident(ctypes.c_uint64(handle), ctypes.c_uint64(scalars_handle), int(montgomery),
                                        d_out.ptr))
    return d_out


def msm_shard_stats() -> dict:
    """bytes moved between device contexts (or from the host) by sharded MSMs since init, sharded calls, replications"""
    a, b, c, d = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_msm_shard_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    return {"scalar_bytes": a.value, "partial_bytes": b.value, "sharded_calls": c.value, "replications": d.value}


def device_peer_info(slot_a: int, slot_b: int) -> int:
    """1: direct peer access between the two contexts' devices, 0: none (copies staged by the runtime), 2: same device"""
    x = ctypes.c_int(-1)
    check(load().capgpu_device_peer_info(slot_a, slot_b, ctypes.byref(x)))
    return x.value


def msm_plan(handle: int, n: int, count: int = 1) -> dict:
    """Which table / sort / split `count` MSMs of n points would take: {'c': 15, 'windows': 18, 'sort': 'two-level',
    'parts': 256, 'n_sub': 65536, 'slice': 1}."""
    buf = ctypes.create_string_buffer(256)
    check(load().capgpu_msm_plan(ctypes.c_uint64(handle), ctypes.c_size_t(n), count, buf, ctypes.c_size_t(256)))
    out = {}
    for kv in buf.value.decode().split():
        if "=" not in kv:
            continue
        k, v = kv.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


# ---- one-shot MSM over caller points (no SRS handle, no table) ---------------------------------------------------
def msm_g1_var(bases: np.ndarray, scalars: np.ndarray, montgomery: bool = True) -> np.ndarray:
    """bases (n, 8) uint64 packed affine points - or (n, 72) uint8: arkworks' GroupAffine with its infinity byte -,
    scalars (n, 4) canonical -> Jacobian (12,) Montgomery.  Nothing stays on the device."""
    bases = np.ascontiguousarray(bases)
    if bases.dtype == np.uint8:
        bases = bases.reshape(-1, 72)
        stride = 72
    else:
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 8)
        stride = 64
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    assert bases.shape[0] == scalars.shape[0]
    out = np.zeros(12, dtype=np.uint64)
    check(load().capgpu_msm_g1_var(bases.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(stride), int(montgomery),
                                   _p(scalars), ctypes.c_size_t(scalars.shape[0]), _p(out)))
    return out


def msm_g1_var_batch(bases_list, scalar_list) -> np.ndarray:
    """one MSM per (bases, scalars) pair, each over its own points, in one pass of launches -> (count, 12)"""
    cnt = len(scalar_list)
    assert len(bases_list) == cnt
    pts = [np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 8) for b in bases_list]
    arrs = [np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4) for s in scalar_list]
    assert all(p.shape[0] == a.shape[0] for p, a in zip(pts, arrs))
    ns = (ctypes.c_size_t * cnt)(*[a.shape[0] for a in arrs])
    bptrs = (u64p * cnt)(*[_p(p) for p in pts])
    sptrs = (u64p * cnt)(*[_p(a) for a in arrs])
    out = np.zeros((cnt, 12), dtype=np.uint64)
    check(load().capgpu_msm_g1_var_batch(bptrs, sptrs, ns, cnt, _p(out)))
    return out


def msm_g1_var_dev(d_bases: DevBuf, d_scalars: DevBuf, n: int, count: int = 1, stride: int | None = None,
                   montgomery: bool = False, d_out: DevBuf | None = None) -> DevBuf:
    """`count` MSMs over the same n device-resident points (packed Montgomery affine); results stay on the device"""
    if d_out is None:
        d_out = DevBuf(96 * count)
    check(load().capgpu_msm_g1_var_dev(d_bases.ptr, d_scalars.ptr, ctypes.c_size_t(n if stride is None else stride),
                                       ctypes.c_size_t(n), count, int(montgomery), d_out.ptr))
    return d_out


def msm_var_plan(n: int, count: int = 1) -> dict:
    """How `count` one-shot MSMs of n points would run: {'path': 'bucket', 'c': 13, 'windows': 20, 'n_sub': 65536,
    'parts': 1, 'sub_msms': 20, 'ranges': 1, 'slice': 1, 'tail': 'horner-quad', 'workspace_bytes': ...}; no device needed."""
    buf = ctypes.create_string_buffer(256)
    check(load().capgpu_msm_var_plan(ctypes.c_size_t(n), count, buf, ctypes.c_size_t(256)))
    out = {}
    for kv in buf.value.decode().split():
        if "=" not in kv:
            continue
        k, v = kv.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


def msm_tail_plan(c: int, n_sub: int, sub_msms: int = 1, has_parts: bool = False) -> dict:
    """What one launch of `sub_msms` sub-MSMs of n_sub points on the c-bit table runs after its plan is chosen (the inputs
    are cg.msm_plan's c, n_sub and count * parts): {'items': 'chained', 'scan': 'one-block', 'digits': 13, 'acc':
    'one-shot', 'acc_grid': ..., 'item_len': ..., 'combine': 'quad', 'combine_lanes': 4, 'reduce': 'grid-quad', ...,
    'partial_points': ..., 'partial_reserved': ...}; no device needed.  The environment switches are read once per
    process."""
    buf = ctypes.create_string_buffer(1024)
    check(load().capgpu_msm_tail_plan(int(c), ctypes.c_size_t(n_sub), int(sub_msms), int(bool(has_parts)), buf,
                                      ctypes.c_size_t(1024)))
    out = {}
    for kv in buf.value.decode().split():
        if "=" not in kv:
            continue
        k, v = kv.split("=")
        out[k] = int(v) if v.isdigit() else v
    return out


# ---- multi-GPU (one process per GPU; RCCL inside the library) -----------------------------------------------------
def comm_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * 128)()
    check(load().capgpu_comm_unique_id(buf))
    return bytes(buf)


def comm_init(rank: int, world: int, unique_id: bytes):
    assert len(unique_id) == 128
    check(load().capgpu_comm_init(rank, world, (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)))


def comm_init_loopback(world: int):
    """test communicator: this process plays `world` ranks one after the other (capgpu.h)"""
    check(load().capgpu_comm_init_loopback(int(world)))


def comm_loopback_set_rank(rank: int):
    check(load().capgpu_comm_loopback_set_rank(int(rank)))


def comm_destroy():
    check(load().capgpu_comm_destroy())


def comm_info():
    r, w = ctypes.c_int(0), ctypes.c_int(0)
    check(load().capgpu_comm_info(ctypes.byref(r), ctypes.byref(w)))
    return r.value, w.value


def msm_g1_sharded_dev(handle: int, d_scalars: DevBuf, n_local: int, count: int = 1, stride: int | None = None,
                       montgomery: bool = False, offset: int = 0, d_out: DevBuf | None = None) -> DevBuf:
    if d_out is None:
        d_out = DevBuf(96 * count)
    check(load().capgpu_msm_g1_sharded_dev(ctypes.c_uint64(handle), ctypes.c_size_t(offset), d_scalars.ptr,
                                           ctypes.c_size_t(n_local if stride is None else stride),
                                           ctypes.c_size_t(n_local), count, int(montgomery), d_out.ptr))
    return d_out


def msm_g1_sharded(handle: int, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    out = np.zeros(12, dtype=np.uint64)
    check(load().capgpu_msm_g1_sharded(ctypes.c_uint64(handle), ctypes.c_size_t(offset),
                                       _p(scalars) if scalars.size else None, ctypes.c_size_t(scalars.shape[0]),
                                       _p(out)))
    return out


def plonk_shard_msm(on: bool):
    check(load().capgpu_plonk_shard_msm(int(on)))


def g1_sum(points: np.ndarray) -> np.ndarray:
    """(k, 12) Jacobian points -> their group sum (12,)."""
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, dtype=np.uint64)
    check(load().capgpu_g1_sum(_p(points.reshape(-1)), ctypes.c_size_t(points.shape[0]), _p(out)))
    return out


# ---- NTT -----------------------------------------------------------------------------------------
def ntt_fr(data: np.ndarray, log_n: int, inverse: bool = False, coset: bool = False) -> np.ndarray:
    data = np.ascontiguousarray(data, dtype=np.uint64).copy()
    assert data.size == 4 << log_n
    check(load().capgpu_ntt_fr(_p(data), ctypes.c_uint32(log_n), int(inverse), int(coset)))
    return data


def ntt_fr_batch(arrays, log_n: int, inverse: bool = False, coset: bool = False):
    arrs = [np.ascontiguousarray(a, dtype=np.uint64).copy() for a in arrays]
    ptrs = (u64p * len(arrs))(*[_p(a) for a in arrs])
    check(load().capgpu_ntt_fr_batch(ptrs, len(arrs), ctypes.c_uint32(log_n), int(inverse), int(coset)))
    return arrs


def ntt_fr_dev(d_data: DevBuf, log_n: int, count: int = 1, stride: int | None = None, inverse: bool = False,
               coset: bool = False):
    check(load().capgpu_ntt_fr_dev(d_data.ptr, ctypes.c_size_t((1 << log_n) if stride is None else stride), count,
                                   ctypes.c_uint32(log_n), int(inverse), int(coset)))


class NttPlanInfo(ctypes.Structure):
    """capgpu_ntt_plan_info (include/capgpu.h)"""
    _fields_ = [("passes", ctypes.c_uint32), ("tile_log", ctypes.c_uint32), ("digits", ctypes.c_uint32 * 3),
                ("log_c", ctypes.c_uint32 * 3), ("tiles", ctypes.c_uint64 * 3), ("persistent", ctypes.c_uint32 * 3),
                ("reserved", ctypes.c_uint32)]


def ntt_plan(log_n: int, count: int = 1) -> dict:
    """How `count` transforms of 2^log_n elements in one call are launched: {'passes': 2, 'tile_log': 10,
    'digits': [6, 6], 'log_c': [4, 4], 'tiles': [4, 4], 'persistent': [False, False]}, one entry per pass in the order
    they run (the row pass last); no device needed."""
    info = NttPlanInfo()
    check(load().capgpu_ntt_plan(ctypes.c_uint32(log_n), count, ctypes.byref(info)))
    k = info.passes
    return {"passes": k, "tile_log": info.tile_log, "digits": list(info.digits)[:k], "log_c": list(info.log_c)[:k],
            "tiles": list(info.tiles)[:k], "persistent": [bool(x) for x in list(info.persistent)[:k]]}


# ---- instrumentation ---------------------------------------------------------------------------
def ubench_mad_rate() -> float:
    """measured v_mad_u64_u32 lane-operations per second of the bound device"""
    out = ctypes.c_double(0)
    check(load().capgpu_ubench_mad_rate(ctypes.byref(out)))
    return out.value


ISSUE_CLASSES = ("v_mad_u64_u32", "v_add_u32", "v_and_b32", "v_mov_b32", "v_lshl_add_u64", "v_lshrrev_b64",
                 "v_alignbit_b32", "v_mul_lo_u32", "mixed_3mad_1plain", "mixed_3mad_1plain_at_3_waves_per_simd")


def ubench_issue_rates() -> dict:
    """measured issue rate (lane-operations per second) of each instruction class, at equal occupancy"""
    out = (ctypes.c_double * len(ISSUE_CLASSES))()
    check(load().capgpu_ubench_issue_rates(out, len(ISSUE_CLASSES)))
    return dict(zip(ISSUE_CLASSES, [float(v) for v in out]))


def profile_enable(on: bool):
    check(load().capgpu_profile_enable(int(on)))


def profile_reset():
    check(load().capgpu_profile_reset())


def profile_stats() -> dict:
    buf = ctypes.create_string_buffer(1 << 16)
    check(load().capgpu_profile_dump(buf, ctypes.c_size_t(len(buf))))
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, cnt = line.split()
        out[name] = (float(ms), int(cnt))
    return out


# ---- PLONK ---------------------------------------------------------------------------------------
INPUT_EVALS, INPUT_COEFFS, INPUT_VARS = 0, 1, 2  # CAPGPU_INPUT_* of include/capgpu.h


def _form(input_form) -> int:
    """'evals' / 'coeffs' / 'vars' / 0 / 1 / 2 -> the ABI's input_form integer (anything else is passed on for the
    library to refuse)"""
    if isinstance(input_form, str):
        return {"evals": INPUT_EVALS, "coeffs": INPUT_COEFFS, "vars": INPUT_VARS}[input_form]
    return int(input_form)


def _wires_per_proof(pk_handles, n: int, input_form) -> int | None:
    """field elements of `wires` per proof: 5 n, or - variable form - the largest num_vars among the keys.  None: a key
    without a table was asked for the variable form; the library refuses the call itself."""
    if _form(input_form) != INPUT_VARS:
        return NUM_WIRE_TYPES * n
    nv = [_cached_num_vars(h) for h in set(pk_handles)]
    return None if 0 in nv else max(nv)


def plonk_preprocess(srs_handle: int, n: int, num_inputs: int, selectors: np.ndarray, sigma_evals: np.ndarray,
                     input_form=INPUT_EVALS):
    """selectors (13, n, 4), sigma_evals (5, n, 4) Montgomery -> (pk handle, VerifyingKey).  input_form = 'coeffs':
    the 18 columns are polynomials in coefficient form (capgpu_plonk_preprocess_ex)."""
    selectors = np.ascontiguousarray(selectors, dtype=np.uint64)
    sigma_evals = np.ascontiguousarray(sigma_evals, dtype=np.uint64)
    assert selectors.size == NUM_SELECTORS * n * 4 and sigma_evals.size == NUM_WIRE_TYPES * n * 4
    h = ctypes.c_uint64()
    vk = VerifyingKey()
    check(load().capgpu_plonk_preprocess_ex(ctypes.c_uint64(srs_handle), ctypes.c_size_t(n),
                                            ctypes.c_size_t(num_inputs), _p(selectors.reshape(-1)),
                                            _p(sigma_evals.reshape(-1)), ctypes.c_int(_form(input_form)),
                                            ctypes.byref(h), ctypes.byref(vk)))
    return h.value, vk


def plonk_preprocess_vars(srs_handle: int, n: int, num_inputs: int, selectors: np.ndarray, wire_vars: np.ndarray,
                          num_vars: int, selector_form=INPUT_EVALS):
    """capgpu_plonk_preprocess_vars: selectors (13, n, 4) in selector_form, wire_vars (5, n) ids below num_vars - the
    circuit's wire -> variable table; the permutation is built on the device -> (pk handle, VerifyingKey).  The key keeps
    the table and proves from input_form='vars'."""
    selectors = np.ascontiguousarray(selectors, dtype=np.uint64)
    wire_vars = np.asarray(wire_vars)
    if wire_vars.size and (wire_vars.min() < 0 or wire_vars.max() > 0xFFFFFFFF):
        raise CapGpuError(-1, "wire_vars ids must fit 32 bits")
    wire_vars = np.ascontiguousarray(wire_vars, dtype=np.uint32)
    assert selectors.size == NUM_SELECTORS * n * 4 and wire_vars.size == NUM_WIRE_TYPES * n
    h = ctypes.c_uint64()
    vk = VerifyingKey()
    check(load().capgpu_plonk_preprocess_vars(ctypes.c_uint64(srs_handle), ctypes.c_size_t(n),
                                              ctypes.c_size_t(num_inputs), _p(selectors.reshape(-1)),
                                              ctypes.c_int(_form(selector_form)),
                                              wire_vars.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                              ctypes.c_size_t(num_vars), ctypes.byref(h), ctypes.byref(vk)))
    return h.value, vk


def plonk_key_set_vars(pk_handle: int, wire_vars: np.ndarray, num_vars: int):
    """capgpu_plonk_key_set_vars: attach the wire -> variable table (5, n) to a key made without one; refused (-1) when
    the permutation it implies is not the key's."""
    n = plonk_key_info(pk_handle)[0]
    wire_vars = np.asarray(wire_vars)
    if wire_vars.size and (wire_vars.min() < 0 or wire_vars.max() > 0xFFFFFFFF):
        raise CapGpuError(-1, "wire_vars ids must fit 32 bits")
    wire_vars = np.ascontiguousarray(wire_vars, dtype=np.uint32)
    if wire_vars.size != NUM_WIRE_TYPES * n:
        raise CapGpuError(-1, f"wire_vars holds {wire_vars.size} ids, key (n = {n}) needs 5 * n")
    _num_vars_of.pop(pk_handle, None)
    check(load().capgpu_plonk_key_set_vars(ctypes.c_uint64(pk_handle),
                                           wire_vars.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                           ctypes.c_size_t(num_vars)))


_num_vars_of = {}  # pk handle -> num_vars of its table, for the shape checks of variable-form calls (handles are never
                   # reused; plonk_key_set_vars and plonk_free_key drop the entry; keys without a table are not cached)


def plonk_key_num_vars(pk_handle: int) -> int:
    """length of an input_form='vars' witness under this key; 0: the key has no variable table"""
    nv = ctypes.c_size_t(0)
    check(load().capgpu_plonk_key_num_vars(ctypes.c_uint64(pk_handle), ctypes.byref(nv)))
    return nv.value


class SolverInfo(ctypes.Structure):
    """capgpu_solver_info (include/capgpu.h): the figures of a key's solver schedule; all zero: the key has none."""
    _fields_ = [("num_given", ctypes.c_uint64), ("num_defined", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("widest_level", ctypes.c_uint64), ("inv_rows", ctypes.c_uint64), ("root_rows", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class SolveStatus(ctypes.Structure):
    """capgpu_solve_status: kind 0 solved, 1 the denominator of `row` (the lowest such row) is zero"""
    _fields_ = [("kind", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("row", ctypes.c_uint64)]


def plonk_key_set_given(pk_handle: int, given_vars) -> SolverInfo:
    """capgpu_plonk_key_set_given: the ids of the variables a caller supplies; the key (one with a wire -> variable
    table) derives the schedule by which capgpu_plonk_solve_vars computes every other variable.  Refused (-1), naming the
    lowest offending row, when the circuit does not follow from the list by the rule of include/capgpu.h."""
    g = np.asarray(given_vars)
    if g.size and (g.min() < 0 or g.max() > 0xFFFFFFFF):
        raise CapGpuError(-1, "given_vars ids must fit 32 bits")
    g = np.ascontiguousarray(g, dtype=np.uint32).reshape(-1)
    info = SolverInfo()
    check(load().capgpu_plonk_key_set_given(ctypes.c_uint64(pk_handle), g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                            ctypes.c_size_t(g.size), ctypes.byref(info)))
    return info


def plonk_key_solver_info(pk_handle: int) -> SolverInfo:
    info = SolverInfo()
    check(load().capgpu_plonk_key_solver_info(ctypes.c_uint64(pk_handle), ctypes.byref(info)))
    return info


HINT_BITS, HINT_INV0, HINT_ISZERO = 0, 1, 2  # CAPGPU_HINT_*


class Hint(ctypes.Structure):
    """capgpu_hint: `count` targets, targets[first .. first + count), valued from the variable src"""
    _fields_ = [("kind", ctypes.c_uint32), ("src", ctypes.c_uint32), ("first", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class HintInfo(ctypes.Structure):
    """capgpu_hint_info: the figures of a key's solver hints; all zero: the key has none."""
    _fields_ = [("num_hints", ctypes.c_uint64), ("num_hinted", ctypes.c_uint64), ("bits_hints", ctypes.c_uint64),
                ("inv_hints", ctypes.c_uint64), ("iszero_hints", ctypes.c_uint64), ("hint_items", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def _solver_lists(given_vars, hints):
    """the given list and a hint list - (kind, src, [targets]) entries - as the set-up calls take them ->
    (ids array, capgpu_hint table, number of hints, target ids array, number of targets)"""
    g = np.asarray(given_vars)
    if g.size and (g.min() < 0 or g.max() > 0xFFFFFFFF):
        raise CapGpuError(-1, "given_vars ids must fit 32 bits")
    g = np.ascontiguousarray(g, dtype=np.uint32).reshape(-1)
    hints = list(hints)
    table = (Hint * max(len(hints), 1))()
    flat = []
    for i, (kind, src, tg) in enumerate(hints):
        tg = [int(t) for t in tg]
        if not (0 <= int(kind) <= 0xFFFFFFFF and 0 <= int(src) <= 0xFFFFFFFF and all(0 <= t <= 0xFFFFFFFF for t in tg)):
            raise CapGpuError(-1, f"hint {i}: kind, src and targets must fit 32 bits")
        table[i] = Hint(int(kind), int(src), len(flat), len(tg))
        flat.extend(tg)
    if len(flat) > 0xFFFFFFFF:
        raise CapGpuError(-1, "the hints' targets must number below 2^32")
    t = np.ascontiguousarray(flat if flat else [0], dtype=np.uint32)
    return g, table, len(hints), t, len(flat)


def plonk_key_set_given_hints(pk_handle: int, given_vars, hints):
    """capgpu_plonk_key_set_given_hints: plonk_key_set_given with a hint list.  hints: (kind, src, [targets]) entries -
    HINT_BITS (target i = bit i of the value of src, 1 .. 254 targets), HINT_INV0 (one target: 1 / src, 0 for 0),
    HINT_ISZERO (one target: 1 if src is 0, else 0) - in the order in which the circuit's builder made them.  The targets
    need not be given: the solver computes them on the device when their source has its value (the rule: include/capgpu.h).
    -> (SolverInfo, HintInfo).  Refused (-1), naming the hint's index and the variable, or the lowest offending row."""
    g, table, num_hints, t, num_targets = _solver_lists(given_vars, hints)
    info, hinfo = SolverInfo(), HintInfo()
    check(load().capgpu_plonk_key_set_given_hints(
        ctypes.c_uint64(pk_handle), g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_size_t(g.size), table,
        ctypes.c_size_t(num_hints), t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_size_t(num_targets),
        ctypes.byref(info), ctypes.byref(hinfo)))
    return info, hinfo


def plonk_key_hint_info(pk_handle: int) -> HintInfo:
    info = HintInfo()
    check(load().capgpu_plonk_key_hint_info(ctypes.c_uint64(pk_handle), ctypes.byref(info)))
    return info


SOLVER_LINEAR, SOLVER_DERIVE_PUBLIC = 1, 2  # CAPGPU_SOLVER_*


class SolverRulesInfo(ctypes.Structure):
    """capgpu_solver_rules_info: the flags a key's solver was set with, its LIN rows and the public-input rows whose
    variable the solver derives; all zero: no solver."""
    _fields_ = [("flags", ctypes.c_uint64), ("lin_rows", ctypes.c_uint64), ("derived_inputs", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def plonk_key_set_solver(pk_handle: int, given_vars, hints=(), flags: int = 0):
    """capgpu_plonk_key_set_solver: plonk_key_set_given_hints under `flags` - SOLVER_LINEAR admits rows that define a
    variable on an input wire through its linear term (an enforce_equal row read backwards), SOLVER_DERIVE_PUBLIC lets a
    public-input variable get its value from such a row instead of the given list.  flags = 0 is plonk_key_set_given_hints.
    -> (SolverInfo, HintInfo); plonk_key_solver_rules_info has the figures of the flags."""
    g, table, num_hints, t, num_targets = _solver_lists(given_vars, hints)
    if not 0 <= int(flags) <= 0xFFFFFFFF:
        raise CapGpuError(-1, "flags must fit 32 bits")
    info, hinfo = SolverInfo(), HintInfo()
    check(load().capgpu_plonk_key_set_solver(
        ctypes.c_uint64(pk_handle), g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_size_t(g.size), table,
        ctypes.c_size_t(num_hints), t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_size_t(num_targets),
        ctypes.c_uint32(int(flags)), ctypes.byref(info), ctypes.byref(hinfo)))
    return info, hinfo


def plonk_key_solver_rules_info(pk_handle: int) -> SolverRulesInfo:
    info = SolverRulesInfo()
    check(load().capgpu_plonk_key_solver_rules_info(ctypes.c_uint64(pk_handle), ctypes.byref(info)))
    return info


SOLVE_FORM_DIRECT, SOLVE_FORM_DEFERRED = 0, 1  # CAPGPU_SOLVE_FORM_*


class SolveFormInfo(ctypes.Structure):
    """capgpu_solve_form_info: the form of the schedule a key's solver runs and its figures; all zero: no solver."""
    _fields_ = [("form", ctypes.c_uint64), ("deferred_vars", ctypes.c_uint64), ("frac_rows", ctypes.c_uint64),
                ("flush_levels", ctypes.c_uint64), ("flush_items", ctypes.c_uint64), ("levels", ctypes.c_uint64),
                ("inv_levels_direct", ctypes.c_uint64), ("inv_levels_deferred", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def plonk_key_set_solve_form(pk_handle: int, form: int) -> SolveFormInfo:
    """capgpu_plonk_key_set_solve_form: re-derives the schedule of the solver the key holds in `form` - SOLVE_FORM_DIRECT,
    what every set-up call leaves, or SOLVE_FORM_DEFERRED, which carries the variables of OUT rows with q_ecc as pairs
    (numerator, denominator) and inverts a chain's denominators together.  Same vars_out, same statuses."""
    info = SolveFormInfo()
    check(load().capgpu_plonk_key_set_solve_form(ctypes.c_uint64(pk_handle), ctypes.c_int(int(form)), ctypes.byref(info)))
    return info


def plonk_key_solve_form_info(pk_handle: int) -> SolveFormInfo:
    info = SolveFormInfo()
    check(load().capgpu_plonk_key_solve_form_info(ctypes.c_uint64(pk_handle), ctypes.byref(info)))
    return info


def plonk_pub_inputs(pk_handle: int, vars_, count: int = 1, out: "DevBuf | None" = None):
    """capgpu_plonk_pub_inputs[_dev]: the public inputs of `count` completed assignments - for every row below num_inputs
    the value that makes the row hold.  vars_: (count, num_vars, 4) Montgomery words -> a (count, num_inputs, 4) array; or a
    DevBuf of that content -> `out` (a DevBuf of count * num_inputs * 32 bytes, allocated here when None), written by a
    launch on the context's stream - not waited for.  The key needs a variable table, not a solver."""
    nv, ni = plonk_key_num_vars(pk_handle), plonk_key_info(pk_handle)[1]
    if count < 0:
        raise CapGpuError(-1, f"count must be >= 0, got {count}")
    L = load()
    if isinstance(vars_, DevBuf):
        if nv and vars_.nbytes < count * nv * 32:
            raise CapGpuError(-1, f"vars holds {vars_.nbytes // 32} field elements, need count * {nv}")
        if out is None:
            out = DevBuf(max(count * ni * 32, 32))
        elif out.nbytes < count * ni * 32:
            raise CapGpuError(-1, f"out holds {out.nbytes} bytes, need count * num_inputs * 32 = {count * ni * 32}")
        check(L.capgpu_plonk_pub_inputs_dev(ctypes.c_uint64(pk_handle), ctypes.c_int(count), vars_.ptr, out.ptr))
        return out
    a = np.ascontiguousarray(vars_, dtype=np.uint64).reshape(-1)
    if nv and a.size != count * nv * 4:
        raise CapGpuError(-1, f"vars holds {a.size / 4:g} field elements, need count * {nv}")
    res = np.zeros((count, ni, 4), np.uint64)
    check(L.capgpu_plonk_pub_inputs(ctypes.c_uint64(pk_handle), ctypes.c_int(count), _p(a) if a.size else None,
                                    _p(res.reshape(-1)) if res.size else None))
    return res


def plonk_solve_vars(pk_handle: int, given, count: int = 1, out: "DevBuf | None" = None):
    """capgpu_plonk_solve_vars[_dev]: completes `count` assignments from their given values.  given: (count, num_given, 4)
    Montgomery words in the order of the key's given list - a numpy array, or a DevBuf of that content.
    -> (vars, [SolveStatus] * count): vars is a (count, num_vars, 4) array for host input; for a DevBuf it is `out` (a
    DevBuf of count * num_vars * 32 bytes, allocated here when None), ready for input_form='vars'."""
    info, nv = plonk_key_solver_info(pk_handle), plonk_key_num_vars(pk_handle)
    if info.num_given == 0 and info.num_defined == 0 and info.levels == 0:
        raise CapGpuError(-1, "capgpu_plonk_solve_vars: the key has no solver (plonk_key_set_given gives it one)")
    if count < 0:
        raise CapGpuError(-1, f"count must be >= 0, got {count}")
    status = (SolveStatus * max(count, 1))()
    L = load()
    if isinstance(given, DevBuf):
        if given.nbytes != count * info.num_given * 32:
            raise CapGpuError(-1, f"given holds {given.nbytes // 32} field elements, need count * {info.num_given}")
        if out is None:
            out = DevBuf(max(count * nv * 32, 32))
        elif out.nbytes < count * nv * 32:
            raise CapGpuError(-1, f"out holds {out.nbytes} bytes, need count * num_vars * 32 = {count * nv * 32}")
        check(L.capgpu_plonk_solve_vars_dev(ctypes.c_uint64(pk_handle), count, given.ptr, out.ptr, status))
        return out, list(status)[:count]
    given = np.ascontiguousarray(given, dtype=np.uint64).reshape(-1)
    if given.size != count * info.num_given * 4:
        raise CapGpuError(-1, f"given holds {given.size / 4:g} field elements, need count * {info.num_given}")
    if given.size == 0:
        given = np.zeros(4, np.uint64)
    vars_out = np.zeros((count, nv, 4), np.uint64)
    check(L.capgpu_plonk_solve_vars(ctypes.c_uint64(pk_handle), count, _p(given), _p(vars_out.reshape(-1)) if count else None,
                                    status))
    return vars_out, list(status)[:count]


def plonk_set_solve_pack(w: int):
    """capgpu_plonk_set_solve_pack: witnesses per workgroup of the solver's launches - 1, 2, 4, 8 or 16; 0 (the default)
    chooses from the key's schedule and the launch's count.  Works before init()."""
    check(load().capgpu_plonk_set_solve_pack(ctypes.c_int(int(w))))


def plonk_get_solve_pack() -> int:
    w = ctypes.c_int(0)
    check(load().capgpu_plonk_get_solve_pack(ctypes.byref(w)))
    return w.value


def plonk_solve_stats() -> dict:
    """counters since init: solver launches, the witnesses they completed, launches at more than one witness per workgroup"""
    a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_solve_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return {"launches": a.value, "witnesses": b.value, "packed_launches": c.value}


INVERSE_FERMAT, INVERSE_GCD = 0, 1
_INVERSE_FORMS = {"fermat": INVERSE_FERMAT, "gcd": INVERSE_GCD}


def fr_set_inverse_form(form):
    """capgpu_fr_set_inverse_form: the form of the Fr inversions in the solver's launches and the batch inverse calls -
    'fermat' / INVERSE_FERMAT (x^(r - 2), the default) or 'gcd' / INVERSE_GCD (constant-time GCD in jumps of divsteps).
    Same results either way.  Works before init()."""
    check(load().capgpu_fr_set_inverse_form(ctypes.c_int(int(_INVERSE_FORMS.get(form, form)))))


def fr_get_inverse_form() -> int:
    f = ctypes.c_int(0)
    check(load().capgpu_fr_get_inverse_form(ctypes.byref(f)))
    return f.value


def fr_inverse_batch(x, out: "DevBuf | None" = None, count: "int | None" = None):
    """capgpu_fr_inverse_batch[_dev]: 1 / x element by element (0 for 0), canonical Montgomery words.  x: an (N, 4) uint64
    array -> a new (N, 4) array; or a DevBuf of `count` elements (all of it when None) -> `out` (x itself when None: in
    place), written by a launch on the context's stream - not waited for."""
    L = load()
    if isinstance(x, DevBuf):
        n = x.nbytes // 32 if count is None else int(count)
        dst = x if out is None else out
        if n < 0 or x.nbytes < n * 32 or dst.nbytes < n * 32:
            raise CapGpuError(-1, f"fr_inverse_batch: {n} elements need {n * 32} bytes in both buffers")
        check(L.capgpu_fr_inverse_batch_dev(x.ptr, dst.ptr, ctypes.c_size_t(n)))
        return dst
    a = np.ascontiguousarray(x, dtype=np.uint64)
    if a.size % 4:
        raise CapGpuError(-1, "fr_inverse_batch: field elements are 4 uint64 words each")
    res = np.zeros_like(a)
    if a.size:
        check(L.capgpu_fr_inverse_batch(_p(a.reshape(-1)), _p(res.reshape(-1)), ctypes.c_size_t(a.size // 4)))
    return res


def fr_inverse_stats() -> dict:
    """launches holding an Fr inversion (solver and batch calls) by the form they ran in, since the library was loaded"""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_fr_inverse_stats(ctypes.byref(a), ctypes.byref(b)))
    return {"fermat_launches": a.value, "gcd_launches": b.value}


def _cached_num_vars(pk_handle: int) -> int:
    nv = _num_vars_of.get(pk_handle)
    if nv is None:
        nv = plonk_key_num_vars(pk_handle)
        if nv:
            _num_vars_of[pk_handle] = nv
    return nv


def plonk_input_stats() -> dict:
    """bytes of witness input copied host -> device by prove and check calls, and launches of the variable form's gather"""
    b, g = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_input_stats(ctypes.byref(b), ctypes.byref(g)))
    return {"witness_bytes_h2d": b.value, "gather_launches": g.value}


def plonk_key_info(pk_handle: int):
    """-> (domain size n, number of public inputs, SRS handle) of a resident proving key."""
    n, ni, srs = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_key_info(ctypes.c_uint64(pk_handle), ctypes.byref(n), ctypes.byref(ni), ctypes.byref(srs)))
    return n.value, ni.value, srs.value


def _check_prove_shapes(pk_handle: int, count: int, wires_elems, pub_inputs: np.ndarray, blinders: np.ndarray,
                        input_form=INPUT_EVALS) -> int:
    """The C ABI takes bare pointers: a mis-shaped array would be read out of bounds.  Every size is checked against
    the key here (wires: count * 5 * n elements - variable form: count * num_vars -, pub_inputs: count * num_inputs,
    blinders: count * 13)."""
    n, num_inputs, _ = plonk_key_info(pk_handle)
    if count < 1:
        raise CapGpuError(-1, f"count must be >= 1, got {count}")
    per = _wires_per_proof([pk_handle], n, input_form)
    if per is not None and wires_elems != count * per:
        raise CapGpuError(-1, f"wires hold {wires_elems} field elements, key (n = {n}) needs count * "
                              f"{'num_vars' if _form(input_form) == INPUT_VARS else '5 * n'} = {count * per}")
    if blinders.size != count * 13 * 4:
        raise CapGpuError(-1, f"blinders hold {blinders.size // 4} field elements, need count * 13 = {count * 13}")
    if pub_inputs.size % 4 or pub_inputs.size != count * num_inputs * 4:
        raise CapGpuError(-1, f"pub_inputs hold {pub_inputs.size / 4:g} field elements, key expects count * "
                              f"{num_inputs} = {count * num_inputs}")
    return num_inputs


def plonk_free_key(pk_handle: int):
    _num_vars_of.pop(pk_handle, None)
    check(load().capgpu_plonk_free_key(ctypes.c_uint64(pk_handle)))


def _bytes_arg(b):
    if b is None:
        return None, 0
    buf = (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b)) if len(b) else None
    return buf, len(b)


def plonk_prove_batch(pk_handle: int, wires: np.ndarray, pub_inputs: np.ndarray, blinders: np.ndarray,
                      ext_msg: bytes | None = None, count: int = 1, input_form=INPUT_EVALS):
    """wires (count, 5, n, 4), pub_inputs (count, l, 4), blinders (count, 13, 4), all Montgomery.  input_form =
    'coeffs': wires are the unblinded wire polynomials in coefficient form; 'vars': wires is (count, num_vars, 4), the
    value of every variable (a key with a table: plonk_preprocess_vars / plonk_key_set_vars)."""
    wires = np.ascontiguousarray(wires, dtype=np.uint64)
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    num_inputs = _check_prove_shapes(pk_handle, count, wires.size // 4 if wires.size % 4 == 0 else -1, pub_inputs,
                                     blinders, input_form)
    proofs = (Proof * count)()
    mbuf, mlen = _bytes_arg(ext_msg)
    pub_ptr = _p(pub_inputs) if pub_inputs.size else None
    check(load().capgpu_plonk_prove_batch_ex(ctypes.c_uint64(pk_handle), count, _p(wires.reshape(-1)), pub_ptr,
                                             ctypes.c_size_t(num_inputs), mbuf, ctypes.c_size_t(mlen), _p(blinders),
                                             ctypes.c_int(_form(input_form)), proofs))
    return list(proofs)


def plonk_prove(pk_handle: int, wires: np.ndarray, pub_inputs: np.ndarray, blinders: np.ndarray,
                ext_msg: bytes | None = None, input_form=INPUT_EVALS) -> Proof:
    """capgpu_plonk_prove: ONE proof per call - the entry point many host threads call at once (it coalesces their
    calls into device batches when plonk_set_coalescing is on).  wires (5, n, 4), pub_inputs (l, 4), blinders (13, 4)."""
    wires = np.ascontiguousarray(wires, dtype=np.uint64)
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    num_inputs = _check_prove_shapes(pk_handle, 1, wires.size // 4 if wires.size % 4 == 0 else -1, pub_inputs, blinders,
                                     input_form)
    proof = Proof()
    mbuf, mlen = _bytes_arg(ext_msg)
    check(load().capgpu_plonk_prove_ex(ctypes.c_uint64(pk_handle), _p(wires.reshape(-1)),
                                       _p(pub_inputs) if pub_inputs.size else None, ctypes.c_size_t(num_inputs), mbuf,
                                       ctypes.c_size_t(mlen), _p(blinders), ctypes.c_int(_form(input_form)),
                                       ctypes.byref(proof)))
    return proof


def has_lagrange_commit() -> bool:
    """the library can take round 1's wire commitments from the witness columns (Lagrange-form commit key per proving key)"""
    return hasattr(load(), "capgpu_plonk_set_wire_commit")


def plonk_set_wire_commit_from_evals(on):
    """True: wire commitments as MSMs of the witness VALUES on the key's Lagrange-form commit key; False: from the
    coefficients (jf-plonk's way); None: the library default.  Same group elements, same proof bytes."""
    if not has_lagrange_commit():
        return
    check(load().capgpu_plonk_set_wire_commit(ctypes.c_int(-1 if on is None else (1 if on else 0))))


class WitnessFault(ctypes.Structure):
    """capgpu_witness_fault (include/capgpu.h): the verdict of the witness check for one proof."""
    _fields_ = [
        ("kind", ctypes.c_uint32),       # 0 satisfied, 1 gate, 2 copy constraint
        ("wire", ctypes.c_uint32),
        ("wire2", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("row", ctypes.c_uint64),
        ("row2", ctypes.c_uint64),
        ("gates_failed", ctypes.c_uint64),
        ("copies_failed", ctypes.c_uint64),
    ]

    def __str__(self):
        """the wording of the reference's check_circuit_satisfiability errors ('' when the witness is satisfied)"""
        if self.kind == 1:
            return f"gate {self.row} not satisfied"
        if self.kind == 2:
            return f"copy constraint ({self.wire},{self.row}) -> ({self.wire2},{self.row2}) violated"
        return ""


def plonk_check_witness_batch(pk_handle, wires, pub_inputs: np.ndarray, count: int = 1, input_form=INPUT_EVALS) -> list:
    """One WitnessFault per witness: gates and copy constraints checked on the device before anything is proved.
    wires: (count, 5, n, 4) numpy array (host: the batch is dealt over the contexts) or a DevBuf of that content -
    input_form='vars': (count, num_vars, 4), one value per variable, gathered on the device; only gates can then fail;
    pk_handle: one key, or a list of `count` keys of one domain (capgpu_plonk_check_witness_multi; pub_inputs then has
    rows of the largest public-input count)."""
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    multi = isinstance(pk_handle, (list, tuple))
    shapes = [plonk_key_info(h) for h in (pk_handle if multi else [pk_handle])]
    n, num_inputs = shapes[0][0], max(sh[1] for sh in shapes)
    if multi and len(pk_handle) != count:
        raise CapGpuError(-1, f"{len(pk_handle)} keys for {count} witnesses")
    if count < 1:
        raise CapGpuError(-1, f"count must be >= 1, got {count}")
    elems = wires.nbytes // 32 if isinstance(wires, DevBuf) else np.asarray(wires).size // 4
    per = _wires_per_proof(pk_handle if multi else [pk_handle], n, input_form)
    if per is not None and elems != count * per:
        raise CapGpuError(-1, f"wires hold {elems} field elements, key (n = {n}) needs count * "
                              f"{'num_vars' if _form(input_form) == INPUT_VARS else '5 * n'} = {count * per}")
    if pub_inputs.size != count * num_inputs * 4:
        raise CapGpuError(-1, f"pub_inputs hold {pub_inputs.size / 4:g} field elements, need count * {num_inputs}")
    faults = (WitnessFault * count)()
    pub_ptr = _p(pub_inputs) if pub_inputs.size else None
    L, form = load(), ctypes.c_int(_form(input_form))
    if isinstance(wires, DevBuf):
        if multi:
            raise CapGpuError(-1, "the multi-key check takes host-resident witnesses")
        check(L.capgpu_plonk_check_witness_batch_dev(ctypes.c_uint64(pk_handle), count, wires.ptr, pub_ptr,
                                                     ctypes.c_size_t(num_inputs), form, faults))
        return list(faults)
    wires = np.ascontiguousarray(wires, dtype=np.uint64).reshape(-1)
    if multi:
        handles = (ctypes.c_uint64 * count)(*pk_handle)
        check(L.capgpu_plonk_check_witness_multi(handles, count, _p(wires), pub_ptr, ctypes.c_size_t(num_inputs), form,
                                                 faults))
    else:
        check(L.capgpu_plonk_check_witness_batch(ctypes.c_uint64(pk_handle), count, _p(wires), pub_ptr,
                                                 ctypes.c_size_t(num_inputs), form, faults))
    return list(faults)


def plonk_set_precheck(on: bool):
    """capgpu_plonk_set_precheck: every prove entry point checks its witnesses first (off by default)"""
    check(load().capgpu_plonk_set_precheck(ctypes.c_int(1 if on else 0)))


def plonk_set_compaction(on: bool):
    """capgpu_plonk_set_compaction: outcome calls under the witness check prove only the witnesses the check let through
    (off by default)"""
    check(load().capgpu_plonk_set_compaction(ctypes.c_int(1 if on else 0)))


def plonk_get_compaction() -> bool:
    m = ctypes.c_int(-1)
    check(load().capgpu_plonk_get_compaction(ctypes.byref(m)))
    return bool(m.value)


def plonk_compaction_stats():
    """(calls that ran compacted, proofs they dropped, witness rows handed to k_move_rows) since capgpu_init"""
    a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_compaction_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def plonk_set_coalescing(window_us: int, max_batch: int = 0):
    check(load().capgpu_plonk_set_coalescing(ctypes.c_uint32(window_us), ctypes.c_uint32(max_batch)))


def plonk_graph_stats():
    """(segments captured, segments replayed) of the small-batch hipGraph path since process start"""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_graph_stats(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


TRANSCRIPT_HOST, TRANSCRIPT_DEVICE = 0, 1  # CAPGPU_TRANSCRIPT_* of include/capgpu.h


def plonk_set_transcript(mode):
    """capgpu_plonk_set_transcript: 'host' / 'device' (or the integers) - where the Fiat-Shamir transcript of the next
    prove calls runs.  Process-wide; callable before init.  Same proof bytes either way."""
    if isinstance(mode, str):
        mode = {"host": TRANSCRIPT_HOST, "device": TRANSCRIPT_DEVICE}[mode]
    check(load().capgpu_plonk_set_transcript(ctypes.c_int(int(mode))))


def plonk_get_transcript() -> int:
    m = ctypes.c_int(-1)
    check(load().capgpu_plonk_get_transcript(ctypes.byref(m)))
    return m.value


def plonk_sync_stats():
    """(device batches proved, host waits on the proving stream inside them) since process start"""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_sync_stats(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def keccak256_batch_dev(messages):
    """Keccak-256 of every bytes object of `messages` by the device transcript's sponge (one wavefront per message):
    a list of 32-byte digests."""
    messages = [bytes(m) for m in messages]
    count = len(messages)
    offs = np.zeros(count + 1, dtype=np.uint64)
    if count:
        offs[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    data = np.frombuffer(b"".join(messages) + b"\0", dtype=np.uint8).copy()
    out = np.zeros(32 * max(count, 1), dtype=np.uint8)
    check(load().capgpu_keccak256_batch_dev(data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            offs.ctypes.data_as(u64p), ctypes.c_int(count),
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    return [out[32 * i:32 * i + 32].tobytes() for i in range(count)]


def plonk_coalescing_stats():
    b, p = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_plonk_coalescing_stats(ctypes.byref(b), ctypes.byref(p)))
    return b.value, p.value


def plonk_prove_batch_dev(pk_handle: int, d_wires: DevBuf, pub_inputs: np.ndarray, blinders: np.ndarray,
                          ext_msg: bytes | None = None, count: int = 1, input_form=INPUT_EVALS):
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    num_inputs = _check_prove_shapes(pk_handle, count, d_wires.nbytes // 32 if d_wires.nbytes % 32 == 0 else -1,
                                     pub_inputs, blinders, input_form)
    proofs = (Proof * count)()
    mbuf, mlen = _bytes_arg(ext_msg)
    pub_ptr = _p(pub_inputs) if pub_inputs.size else None
    check(load().capgpu_plonk_prove_batch_dev_ex(ctypes.c_uint64(pk_handle), count, d_wires.ptr, pub_ptr,
                                                 ctypes.c_size_t(num_inputs), mbuf, ctypes.c_size_t(mlen),
                                                 _p(blinders), ctypes.c_int(_form(input_form)), proofs))
    return list(proofs)


def plonk_prove_multi(pk_handles, wires, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                      input_form=INPUT_EVALS):
    """Proofs of several proving keys (one domain size, one SRS) in one device batch: pk_handles[i] is proof i's key.
    wires: (count, 5, n, 4) numpy array or a DevBuf of that content; pub_rows: (count, max_inputs, 4) - a key with fewer
    public inputs uses the first of its row; ext_msgs: one bytes object per proof, or None."""
    count = len(pk_handles)
    shapes = [plonk_key_info(h) for h in pk_handles]
    n = shapes[0][0]
    max_in = max(sh[1] for sh in shapes)
    pub_rows = np.ascontiguousarray(pub_rows, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    if any(sh[0] != n for sh in shapes):
        raise ValueError("plonk_prove_multi: the keys of one batch must share the domain size")
    if pub_rows.size != count * max_in * 4 or blinders.size != count * 13 * 4:
        raise ValueError(f"plonk_prove_multi: pub_rows must hold {count} x {max_in} and blinders {count} x 13 elements")
    handles = (ctypes.c_uint64 * count)(*pk_handles)
    msgs_arg = lens_arg = None
    keep = []
    if ext_msgs is not None:
        if len(ext_msgs) != count:
            raise ValueError("plonk_prove_multi: one message per proof")
        msgs_arg = (ctypes.c_char_p * count)()
        lens_arg = (ctypes.c_size_t * count)()
        for i, m in enumerate(ext_msgs):
            keep.append(bytes(m) if m else b"")
            msgs_arg[i] = keep[-1] if keep[-1] else None
            lens_arg[i] = len(keep[-1])
    proofs = (Proof * count)()
    pub_ptr = _p(pub_rows) if pub_rows.size else None
    per = _wires_per_proof(pk_handles, n, input_form)  # variable form: rows of the largest num_vars among the keys
    if isinstance(wires, DevBuf):
        if per is not None and wires.nbytes != count * per * 32:
            raise ValueError("plonk_prove_multi: the wire buffer does not hold count x 5 x n elements (count x num_vars)")
        check(load().capgpu_plonk_prove_multi_dev_ex(handles, count, wires.ptr, pub_ptr, ctypes.c_size_t(max_in),
                                                     msgs_arg, lens_arg, _p(blinders), ctypes.c_int(_form(input_form)),
                                                     proofs))
    else:
        wires = np.ascontiguousarray(wires, dtype=np.uint64).reshape(-1)
        if per is not None and wires.size != count * per * 4:
            raise ValueError("plonk_prove_multi: wires must hold count x 5 x n elements (count x num_vars)")
        check(load().capgpu_plonk_prove_multi_ex(handles, count, _p(wires), pub_ptr, ctypes.c_size_t(max_in), msgs_arg,
                                                 lens_arg, _p(blinders), ctypes.c_int(_form(input_form)), proofs))
    return list(proofs)


# ---- asynchronous proving: tickets (capgpu_plonk_prove_batch_async / capgpu_wait) ---------------------------------------
ERR_BUSY = -10  # CAPGPU_ERR_BUSY of include/capgpu.h


class Ticket:
    """A batch being proved by a worker thread of the library.  The object keeps the numpy inputs and the output array
    alive - the library borrows them until the ticket is done - and hands the proofs out through wait()."""

    def __init__(self, ticket: int, proofs, keep):
        self.ticket = ticket
        self._proofs = proofs
        self._keep = keep  # the arrays the library reads: referenced until the result has been taken
        self._result = None
        self._consumed = False

    def wait(self, timeout_ms: int | None = None):
        """-> the list of proofs, or None when the batch is not done within timeout_ms (None: no limit; 0: poll).  Raises
        CapGpuError with the proving call's code and message; a second wait after the result was taken raises
        CapGpuError(-4) (CAPGPU_ERR_BAD_HANDLE), as the C ABI does."""
        done = ctypes.c_int(0)
        t = 0xFFFFFFFF if timeout_ms is None else int(timeout_ms)
        rc = load().capgpu_wait(ctypes.c_uint64(self.ticket), ctypes.c_uint32(t), ctypes.byref(done))
        if rc == 0 and not done.value:
            return None
        if (rc != 0 and rc != -4) or done.value:  # the ticket is consumed: nothing is borrowed any more
            self._consumed = True
            self._keep = None
        check(rc)
        return list(self._proofs)

    def __del__(self):
        # a ticket dropped without wait(): the library still reads the inputs and writes the proofs - wait for it
        try:
            if not self._consumed and self._keep is not None:
                done = ctypes.c_int(0)
                load().capgpu_wait(ctypes.c_uint64(self.ticket), ctypes.c_uint32(0xFFFFFFFF), ctypes.byref(done))
        except Exception:
            pass


def plonk_prove_batch_async(pk_handle: int, wires: np.ndarray, pub_inputs: np.ndarray, blinders: np.ndarray,
                            ext_msg: bytes | None = None, count: int = 1, input_form=INPUT_EVALS) -> Ticket:
    """plonk_prove_batch without the wait: returns a Ticket at once; Ticket.wait() gives the proofs.  Keep two in flight
    from one thread to overlap one batch's copies and host steps with the other's kernels."""
    wires = np.ascontiguousarray(wires, dtype=np.uint64)
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    num_inputs = _check_prove_shapes(pk_handle, count, wires.size // 4 if wires.size % 4 == 0 else -1, pub_inputs,
                                     blinders, input_form)
    proofs = (Proof * count)()
    mbuf, mlen = _bytes_arg(ext_msg)
    pub_ptr = _p(pub_inputs) if pub_inputs.size else None
    flat = wires.reshape(-1)
    t = ctypes.c_uint64(0)
    check(load().capgpu_plonk_prove_batch_async(ctypes.c_uint64(pk_handle), count, _p(flat), pub_ptr,
                                                ctypes.c_size_t(num_inputs), mbuf, ctypes.c_size_t(mlen), _p(blinders),
                                                ctypes.c_int(_form(input_form)), proofs, ctypes.byref(t)))
    return Ticket(t.value, proofs, (wires, flat, pub_inputs, blinders))


def plonk_prove_multi_async(pk_handles, wires: np.ndarray, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                            input_form=INPUT_EVALS) -> Ticket:
    """plonk_prove_multi (host-resident wires) without the wait: a Ticket."""
    count = len(pk_handles)
    shapes = [plonk_key_info(h) for h in pk_handles]
    n = shapes[0][0]
    max_in = max(sh[1] for sh in shapes)
    pub_rows = np.ascontiguousarray(pub_rows, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    wires = np.ascontiguousarray(wires, dtype=np.uint64).reshape(-1)
    if pub_rows.size != count * max_in * 4 or blinders.size != count * 13 * 4:
        raise ValueError(f"plonk_prove_multi_async: pub_rows must hold {count} x {max_in} and blinders {count} x 13 elements")
    per = _wires_per_proof(pk_handles, n, input_form)
    if per is not None and wires.size != count * per * 4:
        raise ValueError("plonk_prove_multi_async: wires must hold count x 5 x n elements (count x num_vars)")
    handles = (ctypes.c_uint64 * count)(*pk_handles)
    msgs_arg = lens_arg = None
    keep = []
    if ext_msgs is not None:
        if len(ext_msgs) != count:
            raise ValueError("plonk_prove_multi_async: one message per proof")
        msgs_arg = (ctypes.c_char_p * count)()
        lens_arg = (ctypes.c_size_t * count)()
        for i, m in enumerate(ext_msgs):
            keep.append(bytes(m) if m else b"")
            msgs_arg[i] = keep[-1] if keep[-1] else None
            lens_arg[i] = len(keep[-1])
    proofs = (Proof * count)()
    pub_ptr = _p(pub_rows) if pub_rows.size else None
    t = ctypes.c_uint64(0)
    check(load().capgpu_plonk_prove_multi_async(handles, count, _p(wires), pub_ptr, ctypes.c_size_t(max_in), msgs_arg,
                                                lens_arg, _p(blinders), ctypes.c_int(_form(input_form)), proofs,
                                                ctypes.byref(t)))
    return Ticket(t.value, proofs, (wires, pub_rows, blinders))


def async_stats() -> dict:
    """tickets accepted / finished since init and the most that ran at once on one device"""
    a, b, m = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    check(load().capgpu_async_stats(ctypes.byref(a), ctypes.byref(b), ctypes.byref(m)))
    return {"submitted": a.value, "completed": b.value, "max_running": m.value}


# ---- per-proof outcomes (capgpu_plonk_prove_each*): a batch is proved past its unsatisfied witnesses ---------------------
ERR_PROOF = -7  # CAPGPU_ERR_PROOF of include/capgpu.h


class ProveOutcome(ctypes.Structure):
    """capgpu_prove_outcome (include/capgpu.h): the verdict of one proof of a prove_each call.  A failed proof's record
    is all-ones words."""
    _fields_ = [
        ("status", ctypes.c_int32),        # 0, or ERR_PROOF: this witness does not satisfy its circuit
        ("degree_flags", ctypes.c_uint32),
        ("fault", WitnessFault),           # precheck on: the check's verdict; off: kind 0
    ]

    def __str__(self):
        return prove_outcome_text(self)


def prove_outcome_text(outcome: ProveOutcome) -> str:
    """capgpu_prove_outcome_text: the message a lone plonk_prove of that witness raises ('' for a proof that was made)"""
    buf = ctypes.create_string_buffer(512)
    check(load().capgpu_prove_outcome_text(ctypes.byref(outcome), buf, ctypes.c_size_t(len(buf))))
    return buf.value.decode()


def _each_args(who: str, pk_handles, wires_elems, pub_rows, blinders, ext_msgs, input_form):
    count = len(pk_handles)
    pub_rows = np.ascontiguousarray(pub_rows, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    max_in = 0
    if count:
        shapes = [plonk_key_info(h) for h in set(pk_handles)]
        n = shapes[0][0]
        max_in = max(sh[1] for sh in shapes)
        if any(sh[0] != n for sh in shapes):
            raise ValueError(f"{who}: the keys of one batch must share the domain size")
        per = None if wires_elems is None else _wires_per_proof(pk_handles, n, input_form)  # (None: no `wires` argument)
        if per is not None and wires_elems != count * per:
            raise ValueError(f"{who}: wires must hold count x 5 x n elements (count x num_vars)")
    if pub_rows.size != count * max_in * 4 or blinders.size != count * 13 * 4:
        raise ValueError(f"{who}: pub_rows must hold {count} x {max_in} and blinders {count} x 13 elements")
    handles = (ctypes.c_uint64 * max(count, 1))(*pk_handles)
    msgs_arg = lens_arg = None
    keep = [pub_rows, blinders]
    if ext_msgs is not None:
        if len(ext_msgs) != count:
            raise ValueError(f"{who}: one message per proof")
        msgs_arg = (ctypes.c_char_p * max(count, 1))()
        lens_arg = (ctypes.c_size_t * max(count, 1))()
        for i, m in enumerate(ext_msgs):
            keep.append(bytes(m) if m else b"")
            msgs_arg[i] = keep[-1] if keep[-1] else None
            lens_arg[i] = len(keep[-1])
    proofs = (Proof * max(count, 1))()
    outcomes = (ProveOutcome * max(count, 1))()
    pub_ptr = _p(pub_rows) if pub_rows.size else None
    return count, handles, pub_ptr, max_in, msgs_arg, lens_arg, blinders, proofs, outcomes, keep


def plonk_prove_each(pk_handles, wires: np.ndarray, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                     input_form=INPUT_EVALS):
    """capgpu_plonk_prove_each: plonk_prove_multi that keeps going past an unsatisfied witness -> (proofs, outcomes),
    one ProveOutcome per proof.  Raises only when the batch could not run.  A proof whose outcome has status 0 is the
    lone plonk_prove's proof; a failed one is all-ones words."""
    wires = np.ascontiguousarray(wires, dtype=np.uint64).reshape(-1)
    count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, _keep = _each_args(
        "plonk_prove_each", list(pk_handles), wires.size // 4, pub_rows, blinders, ext_msgs, input_form)
    check(load().capgpu_plonk_prove_each(handles, count, _p(wires), pub_ptr, ctypes.c_size_t(max_in), msgs, lens,
                                         _p(blinders), ctypes.c_int(_form(input_form)), proofs, outcomes))
    return list(proofs)[:count], list(outcomes)[:count]


def plonk_prove_each_dev(pk_handles, d_wires: DevBuf, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                         input_form=INPUT_EVALS):
    """capgpu_plonk_prove_each_dev: the same from a device buffer, on the calling context's stream."""
    count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, _keep = _each_args(
        "plonk_prove_each_dev", list(pk_handles), d_wires.nbytes // 32, pub_rows, blinders, ext_msgs, input_form)
    check(load().capgpu_plonk_prove_each_dev(handles, count, d_wires.ptr, pub_ptr, ctypes.c_size_t(max_in), msgs, lens,
                                             _p(blinders), ctypes.c_int(_form(input_form)), proofs, outcomes))
    return list(proofs)[:count], list(outcomes)[:count]


class EachTicket(Ticket):
    """The Ticket of plonk_prove_each_async: wait() -> (proofs, outcomes).  The outcome array is borrowed by the library
    like the proofs."""

    def __init__(self, ticket: int, proofs, outcomes, count: int, keep):
        super().__init__(ticket, proofs, keep)
        self._outcomes = outcomes
        self._count = count

    def wait(self, timeout_ms: int | None = None):
        proofs = super().wait(timeout_ms)
        if proofs is None:
            return None
        return proofs[:self._count], list(self._outcomes)[:self._count]


def plonk_prove_each_async(pk_handles, wires: np.ndarray, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                           input_form=INPUT_EVALS) -> EachTicket:
    """capgpu_plonk_prove_each_async: plonk_prove_each without the wait; EachTicket.wait() -> (proofs, outcomes)."""
    wires = np.ascontiguousarray(wires, dtype=np.uint64).reshape(-1)
    count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, keep = _each_args(
        "plonk_prove_each_async", list(pk_handles), wires.size // 4, pub_rows, blinders, ext_msgs, input_form)
    t = ctypes.c_uint64(0)
    check(load().capgpu_plonk_prove_each_async(handles, count, _p(wires), pub_ptr, ctypes.c_size_t(max_in), msgs, lens,
                                               _p(blinders), ctypes.c_int(_form(input_form)), proofs, outcomes,
                                               ctypes.byref(t)))
    return EachTicket(t.value, proofs, outcomes, count, (wires, keep))


# ---- a Vec of notes over keys of several domain sizes (capgpu_plonk_prove_notes*) ---------------------------------------
class NotesGroup(ctypes.Structure):
    """capgpu_notes_group (include/capgpu.h): one group of a notes call - the notes whose keys share domain size and SRS."""
    _fields_ = [("srs_handle", ctypes.c_uint64), ("domain_size", ctypes.c_uint64), ("count", ctypes.c_uint32),
                ("first", ctypes.c_uint32), ("max_inputs", ctypes.c_uint32), ("run_order", ctypes.c_uint32)]


class NotesStats(ctypes.Structure):
    """capgpu_notes_stats (include/capgpu.h)"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("calls", "groups", "groups_dealt", "contexts_dealt", "dev_groups_direct",
                                               "dev_groups_gathered", "rows_gathered")]


def _notes_args(who: str, pk_handles, pub_rows, blinders, ext_msgs):
    """the per-note arrays of a notes call: rows of the largest num_inputs among ALL the keys, 13 blinders per note"""
    count = len(pk_handles)
    pub_rows = np.ascontiguousarray(pub_rows, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    if blinders.size != count * 13 * 4 or (count and pub_rows.size % (4 * count)):
        raise ValueError(f"{who}: pub_rows must hold {count} equal rows and blinders {count} x 13 elements")
    num_inputs = pub_rows.size // (4 * count) if count else 0
    handles = (ctypes.c_uint64 * max(count, 1))(*pk_handles)
    msgs_arg = lens_arg = None
    keep = [pub_rows, blinders]
    if ext_msgs is not None:
        if len(ext_msgs) != count:
            raise ValueError(f"{who}: one message per note")
        msgs_arg = (ctypes.c_char_p * max(count, 1))()
        lens_arg = (ctypes.c_size_t * max(count, 1))()
        for i, m in enumerate(ext_msgs):
            keep.append(bytes(m) if m else b"")
            msgs_arg[i] = keep[-1] if keep[-1] else None
            lens_arg[i] = len(keep[-1])
    proofs = (Proof * max(count, 1))()
    outcomes = (ProveOutcome * max(count, 1))()
    pub_ptr = _p(pub_rows) if pub_rows.size else None
    return count, handles, pub_ptr, num_inputs, msgs_arg, lens_arg, blinders, proofs, outcomes, keep


def _notes_rows(who: str, wires, count: int):
    """one pointer per note: every wires[i] is that note's own block (any uint64 array; a view is read where it is when
    it is contiguous) -> (the pointer array, the arrays to keep alive)"""
    if len(wires) != count:
        raise ValueError(f"{who}: one witness block per note")
    rows = [np.ascontiguousarray(w, dtype=np.uint64).reshape(-1) for w in wires]
    ptrs = (ctypes.c_void_p * max(count, 1))(*[r.ctypes.data for r in rows])
    return ptrs, rows


def plonk_prove_notes(pk_handles, wires, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None, input_form=INPUT_EVALS):
    """capgpu_plonk_prove_notes: prove_each over keys of SEVERAL domain sizes (or SRS) -> (proofs, outcomes).  wires: one
    array per note - 5 n_i elements, or (input_form='vars') the key's num_vars values; pub_rows: count rows of the largest
    num_inputs among all the keys.  Every note's proof and outcome are what plonk_prove_each makes of its group alone."""
    count, handles, pub_ptr, ni, msgs, lens, blinders, proofs, outcomes, _keep = _notes_args(
        "plonk_prove_notes", list(pk_handles), pub_rows, blinders, ext_msgs)
    ptrs, _rows = _notes_rows("plonk_prove_notes", wires, count)
    check(load().capgpu_plonk_prove_notes(handles, count, ptrs, pub_ptr, ctypes.c_size_t(ni), msgs, lens, _p(blinders),
                                          ctypes.c_int(_form(input_form)), proofs, outcomes))
    return list(proofs)[:count], list(outcomes)[:count]


def plonk_prove_notes_dev(pk_handles, d_wires, wire_offsets, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                          input_form=INPUT_EVALS):
    """capgpu_plonk_prove_notes_dev: the same from ONE device buffer (a DevBuf, or a device address), note i's block at
    wire_offsets[i] field elements from its start; on the calling context's stream.  The buffer is never written."""
    count, handles, pub_ptr, ni, msgs, lens, blinders, proofs, outcomes, _keep = _notes_args(
        "plonk_prove_notes_dev", list(pk_handles), pub_rows, blinders, ext_msgs)
    if len(wire_offsets) != count:
        raise ValueError("plonk_prove_notes_dev: one offset per note")
    offs = (ctypes.c_uint64 * max(count, 1))(*[int(o) for o in wire_offsets])
    ptr = d_wires.ptr if isinstance(d_wires, DevBuf) else ctypes.c_void_p(int(d_wires))
    check(load().capgpu_plonk_prove_notes_dev(handles, count, ptr, offs, pub_ptr, ctypes.c_size_t(ni), msgs, lens,
                                              _p(blinders), ctypes.c_int(_form(input_form)), proofs, outcomes))
    return list(proofs)[:count], list(outcomes)[:count]


def plonk_prove_notes_async(pk_handles, wires, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None,
                            input_form=INPUT_EVALS) -> EachTicket:
    """capgpu_plonk_prove_notes_async: plonk_prove_notes without the wait; EachTicket.wait() -> (proofs, outcomes)."""
    count, handles, pub_ptr, ni, msgs, lens, blinders, proofs, outcomes, keep = _notes_args(
        "plonk_prove_notes_async", list(pk_handles), pub_rows, blinders, ext_msgs)
    ptrs, rows = _notes_rows("plonk_prove_notes_async", wires, count)
    t = ctypes.c_uint64(0)
    check(load().capgpu_plonk_prove_notes_async(handles, count, ptrs, pub_ptr, ctypes.c_size_t(ni), msgs, lens, _p(blinders),
                                                ctypes.c_int(_form(input_form)), proofs, outcomes, ctypes.byref(t)))
    return EachTicket(t.value, proofs, outcomes, count, (rows, keep))


def plonk_notes_plan(pk_handles, cap: int | None = None):
    """capgpu_plonk_notes_plan -> (groups, group_of, num_groups): the groups a notes call over these keys forms - at most
    `cap` records (None: all of them) -, every note's group, and the true number of groups."""
    pk_handles = list(pk_handles)
    count = len(pk_handles)
    handles = (ctypes.c_uint64 * max(count, 1))(*pk_handles)
    group_of = (ctypes.c_uint32 * max(count, 1))()
    num = ctypes.c_size_t(0)
    room = count if cap is None else int(cap)
    groups = (NotesGroup * max(room, 1))()
    check(load().capgpu_plonk_notes_plan(handles, count, groups, ctypes.c_size_t(room), ctypes.byref(num), group_of))
    return list(groups)[:min(room, num.value)], list(group_of)[:count], num.value


def plonk_reserve_notes(pk_handles, input_form=INPUT_EVALS, slot: int = -1):
    """capgpu_plonk_reserve_notes: size context `slot` (-1: every one) for a notes call over these keys, host or device form"""
    pk_handles = list(pk_handles)
    handles = (ctypes.c_uint64 * max(len(pk_handles), 1))(*pk_handles)
    check(load().capgpu_plonk_reserve_notes(handles, len(pk_handles), ctypes.c_int(_form(input_form)), ctypes.c_int(slot)))


def plonk_notes_stats() -> dict:
    """capgpu_plonk_notes_stats: process-wide counters of the notes calls since init"""
    s = NotesStats()
    check(load().capgpu_plonk_notes_stats(ctypes.byref(s)))
    return {k: getattr(s, k) for k, _ in NotesStats._fields_}


# ---- proving from given values (capgpu_plonk_prove_given*): the solver and the variable-form outcome call in one ---------
def _given_args(who: str, pk_handles, given_elems, pub_rows, blinders, ext_msgs):
    count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, keep = _each_args(
        who, pk_handles, None, pub_rows, blinders, ext_msgs, INPUT_VARS)
    if count:
        max_given = max(plonk_key_solver_info(h).num_given for h in set(pk_handles))
        if given_elems != count * max_given:
            raise ValueError(f"{who}: given must hold count x {max_given} elements (the largest given list of the keys)")
    solved = (SolveStatus * max(count, 1))()
    return count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, keep


def plonk_prove_given(pk_handles, given, pub_rows: np.ndarray, blinders: np.ndarray, ext_msgs=None):
    """capgpu_plonk_prove_given[_dev]: from the values each circuit is given to proofs, in one call ->
    (proofs, outcomes, solved): one ProveOutcome and one SolveStatus per proof.  given: (count, num_given, 4) Montgomery
    words in the order of the key's given list (several keys: rows of the largest list) - a numpy array, or a DevBuf of
    that content, which is only read.  Proofs and outcomes are those of plonk_solve_vars followed by
    plonk_prove_each_dev(..., input_form='vars')."""
    pk_handles = list(pk_handles)
    L = load()
    if isinstance(given, DevBuf):
        count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, _keep = _given_args(
            "plonk_prove_given", pk_handles, given.nbytes // 32, pub_rows, blinders, ext_msgs)
        check(L.capgpu_plonk_prove_given_dev(handles, count, given.ptr, pub_ptr, ctypes.c_size_t(max_in), msgs, lens,
                                             _p(blinders), proofs, outcomes, solved))
    else:
        given = np.ascontiguousarray(given, dtype=np.uint64).reshape(-1)
        count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, _keep = _given_args(
            "plonk_prove_given", pk_handles, given.size // 4, pub_rows, blinders, ext_msgs)
        if given.size == 0:
            given = np.zeros(4, np.uint64)
        check(L.capgpu_plonk_prove_given(handles, count, _p(given), pub_ptr, ctypes.c_size_t(max_in), msgs, lens,
                                         _p(blinders), proofs, outcomes, solved))
    return list(proofs)[:count], list(outcomes)[:count], list(solved)[:count]


class GivenTicket(EachTicket):
    """The Ticket of plonk_prove_given_async: wait() -> (proofs, outcomes, solved)."""

    def __init__(self, ticket: int, proofs, outcomes, solved, count: int, keep):
        super().__init__(ticket, proofs, outcomes, count, keep)
        self._solved = solved

    def wait(self, timeout_ms: int | None = None):
        r = super().wait(timeout_ms)
        if r is None:
            return None
        return r[0], r[1], list(self._solved)[:self._count]


def plonk_prove_given_async(pk_handles, given: np.ndarray, pub_rows: np.ndarray, blinders: np.ndarray,
                            ext_msgs=None) -> GivenTicket:
    """capgpu_plonk_prove_given_async: plonk_prove_given (host values) without the wait.  Two tickets in flight run one
    batch's solve beside the other's rounds."""
    pk_handles = list(pk_handles)
    given = np.ascontiguousarray(given, dtype=np.uint64).reshape(-1)
    count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, keep = _given_args(
        "plonk_prove_given_async", pk_handles, given.size // 4, pub_rows, blinders, ext_msgs)
    if given.size == 0:
        given = np.zeros(4, np.uint64)
    t = ctypes.c_uint64(0)
    check(load().capgpu_plonk_prove_given_async(handles, count, _p(given), pub_ptr, ctypes.c_size_t(max_in), msgs, lens,
                                                _p(blinders), proofs, outcomes, solved, ctypes.byref(t)))
    return GivenTicket(t.value, proofs, outcomes, solved, count, (given, keep))


def _given_io_args(who: str, pk_handles, given_elems, blinders, ext_msgs):
    """_given_args for the _io calls: no public inputs come in; pub_out - (count, num_inputs, 4), zeroed - is the array the
    library writes them to, and pub_ptr points at IT (None when the keys have no public inputs)"""
    max_in = max((plonk_key_info(h)[1] for h in set(pk_handles)), default=0)
    pub_out = np.zeros((len(pk_handles), max_in, 4), np.uint64)
    count, handles, _, max_in, msgs, lens, blinders, proofs, outcomes, solved, keep = _given_args(
        who, pk_handles, given_elems, pub_out, blinders, ext_msgs)
    pub_ptr = _p(pub_out.reshape(-1)) if pub_out.size else None            # (C-contiguous: reshape is a view of pub_out)
    return count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, keep, pub_out


def plonk_prove_given_io(pk_handles, given, blinders: np.ndarray, ext_msgs=None):
    """capgpu_plonk_prove_given_io[_dev]: plonk_prove_given without public inputs to pass - they are computed on the device
    from each solved assignment and returned -> (proofs, outcomes, solved, pub_inputs), pub_inputs a
    (count, num_inputs, 4) array of Montgomery words: what the proofs verify against."""
    pk_handles = list(pk_handles)
    L = load()
    if isinstance(given, DevBuf):
        count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, _keep, pub_out = _given_io_args(
            "plonk_prove_given_io", pk_handles, given.nbytes // 32, blinders, ext_msgs)
        check(L.capgpu_plonk_prove_given_io_dev(handles, count, given.ptr, ctypes.c_size_t(max_in), msgs, lens, _p(blinders),
                                                pub_ptr, proofs, outcomes, solved))
    else:
        given = np.ascontiguousarray(given, dtype=np.uint64).reshape(-1)
        count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, _keep, pub_out = _given_io_args(
            "plonk_prove_given_io", pk_handles, given.size // 4, blinders, ext_msgs)
        if given.size == 0:
            given = np.zeros(4, np.uint64)
        check(L.capgpu_plonk_prove_given_io(handles, count, _p(given), ctypes.c_size_t(max_in), msgs, lens, _p(blinders),
                                            pub_ptr, proofs, outcomes, solved))
    return list(proofs)[:count], list(outcomes)[:count], list(solved)[:count], pub_out


class GivenIoTicket(GivenTicket):
    """The Ticket of plonk_prove_given_io_async: wait() -> (proofs, outcomes, solved, pub_inputs)."""

    def __init__(self, ticket: int, proofs, outcomes, solved, count: int, keep, pub_out):
        super().__init__(ticket, proofs, outcomes, solved, count, keep)
        self._pub_out = pub_out

    def wait(self, timeout_ms: int | None = None):
        r = super().wait(timeout_ms)
        if r is None:
            return None
        return r + (self._pub_out,)


def plonk_prove_given_io_async(pk_handles, given: np.ndarray, blinders: np.ndarray, ext_msgs=None) -> GivenIoTicket:
    """capgpu_plonk_prove_given_io_async: plonk_prove_given_io (host values) without the wait; the public-input array is
    borrowed by the library like the proofs."""
    pk_handles = list(pk_handles)
    given = np.ascontiguousarray(given, dtype=np.uint64).reshape(-1)
    count, handles, pub_ptr, max_in, msgs, lens, blinders, proofs, outcomes, solved, keep, pub_out = _given_io_args(
        "plonk_prove_given_io_async", pk_handles, given.size // 4, blinders, ext_msgs)
    if given.size == 0:
        given = np.zeros(4, np.uint64)
    t = ctypes.c_uint64(0)
    check(load().capgpu_plonk_prove_given_io_async(handles, count, _p(given), ctypes.c_size_t(max_in), msgs, lens,
                                                   _p(blinders), pub_ptr, proofs, outcomes, solved, ctypes.byref(t)))
    return GivenIoTicket(t.value, proofs, outcomes, solved, count, (given, keep, pub_out), pub_out)


def plonk_reserve_given(pk_handle: int, count: int, slot: int = -1):
    """capgpu_plonk_reserve_given: plonk_reserve(pk, count, 'vars', slot) plus what a plonk_prove_given of `count` proofs
    adds - the staged given values, the solved buffer, the status words, the key's schedule on the context."""
    check(load().capgpu_plonk_reserve_given(ctypes.c_uint64(pk_handle), ctypes.c_int(count), ctypes.c_int(slot)))


def _given_one_args(given, blinders, ext_msg):
    given = np.ascontiguousarray(given, dtype=np.uint64).reshape(-1)
    blinders = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1)
    if given.size % 4 or blinders.size != 13 * 4:
        raise ValueError("plonk_prove_given_one: given is (num_given, 4), blinders (13, 4) words")
    mbuf, mlen = _bytes_arg(ext_msg)
    return given, blinders, mbuf, mlen


def plonk_prove_given_one(pk_handle: int, given: np.ndarray, pub_inputs: np.ndarray, blinders: np.ndarray,
                          ext_msg: bytes | None = None):
    """capgpu_plonk_prove_given_one: ONE proof from the values its circuit is given -> (proof, outcome, solved) - the call
    many host threads make at once: with plonk_set_coalescing on, their calls are gathered into one solve and one batch;
    off, it is plonk_prove_given([pk], ...).  given (num_given, 4), pub_inputs (num_inputs, 4), blinders (13, 4).  The
    library call runs without the GIL, as every call through ctypes does."""
    given, blinders, mbuf, mlen = _given_one_args(given, blinders, ext_msg)
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    proof, outcome, solved = Proof(), ProveOutcome(), SolveStatus()
    check(load().capgpu_plonk_prove_given_one(
        ctypes.c_uint64(pk_handle), _p(given) if given.size else None, ctypes.c_size_t(given.size // 4),
        _p(pub_inputs) if pub_inputs.size else None, ctypes.c_size_t(pub_inputs.size // 4), mbuf, ctypes.c_size_t(mlen),
        _p(blinders), ctypes.byref(proof), ctypes.byref(outcome), ctypes.byref(solved)))
    return proof, outcome, solved


def plonk_prove_given_io_one(pk_handle: int, given: np.ndarray, blinders: np.ndarray, ext_msg: bytes | None = None,
                             num_inputs: int | None = None):
    """capgpu_plonk_prove_given_io_one: plonk_prove_given_one without public inputs to pass -> (proof, outcome, solved,
    pub_inputs), pub_inputs the (num_inputs, 4) Montgomery words the proof verifies against.  num_inputs: the key's
    (None: asked of the key)."""
    given, blinders, mbuf, mlen = _given_one_args(given, blinders, ext_msg)
    if num_inputs is None:
        num_inputs = plonk_key_info(pk_handle)[1]
    pub_out = np.zeros((int(num_inputs), 4), np.uint64)
    proof, outcome, solved = Proof(), ProveOutcome(), SolveStatus()
    check(load().capgpu_plonk_prove_given_io_one(
        ctypes.c_uint64(pk_handle), _p(given) if given.size else None, ctypes.c_size_t(given.size // 4),
        ctypes.c_size_t(int(num_inputs)), mbuf, ctypes.c_size_t(mlen), _p(blinders),
        _p(pub_out.reshape(-1)) if pub_out.size else None, ctypes.byref(proof), ctypes.byref(outcome), ctypes.byref(solved)))
    return proof, outcome, solved, pub_out


def plonk_reserve(pk_handle: int, count: int, input_form=INPUT_EVALS, slot: int = -1):
    """capgpu_plonk_reserve: size context `slot` (-1: all) ahead for a `count`-proof host-resident batch under this key,
    in the modes in force now, without proving anything."""
    check(load().capgpu_plonk_reserve(ctypes.c_uint64(pk_handle), ctypes.c_int(count), ctypes.c_int(_form(input_form)),
                                      ctypes.c_int(slot)))


def scratch_stats() -> dict:
    """growths of scratch buffers / pinned areas since init: events, bytes of new capacity, milliseconds spent"""
    e, b, ms = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_double(0.0)
    check(load().capgpu_scratch_stats(ctypes.byref(e), ctypes.byref(b), ctypes.byref(ms)))
    return {"grow_events": e.value, "grow_bytes": b.value, "grow_ms": ms.value}


def proof_to_arrays(pr: Proof) -> dict:
    """ctypes Proof -> dict of numpy arrays (Montgomery words)."""
    def a(x):
        return np.ctypeslib.as_array(x).copy()
    return {
        "wires_poly_comms": a(pr.wires_poly_comms), "prod_perm_poly_comm": a(pr.prod_perm_poly_comm),
        "split_quot_poly_comms": a(pr.split_quot_poly_comms), "opening_proof": a(pr.opening_proof),
        "shifted_opening_proof": a(pr.shifted_opening_proof), "wires_evals": a(pr.wires_evals),
        "wire_sigma_evals": a(pr.wire_sigma_evals), "perm_next_eval": a(pr.perm_next_eval),
    }


# ---- verification (host only) -------------------------------------------------------------------------
def g2_generator() -> np.ndarray:
    out = np.zeros(16, dtype=np.uint64)
    check(load().capgpu_g2_generator(_p(out)))
    return out


def g2_mul(q: np.ndarray, scalar: int) -> np.ndarray:
    out = np.zeros(16, dtype=np.uint64)
    check(load().capgpu_g2_mul(_p(np.ascontiguousarray(q, dtype=np.uint64)), _limbs(scalar), _p(out)))
    return out


def pairing_check(g1_points: np.ndarray, g2_points: np.ndarray) -> bool:
    g1_points = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, 8)
    g2_points = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, 16)
    ok = ctypes.c_int(0)
    check(load().capgpu_pairing_check(_p(g1_points.reshape(-1)), _p(g2_points.reshape(-1)),
                                      ctypes.c_size_t(g1_points.shape[0]), ctypes.byref(ok)))
    return bool(ok.value)


def plonk_verify(vk: VerifyingKey, g2_h: np.ndarray, g2_beta_h: np.ndarray, pub_inputs: np.ndarray, proof: Proof,
                 ext_msg: bytes | None = None) -> bool:
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    mbuf, mlen = _bytes_arg(ext_msg)
    ok = ctypes.c_int(0)
    check(load().capgpu_plonk_verify(ctypes.byref(vk), _p(np.ascontiguousarray(g2_h, dtype=np.uint64)),
                                     _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64)),
                                     _p(pub_inputs) if pub_inputs.size else None, ctypes.c_size_t(pub_inputs.size // 4),
                                     ctypes.byref(proof), mbuf, ctypes.c_size_t(mlen), ctypes.byref(ok)))
    return bool(ok.value)


def plonk_batch_verify(vks, g2_h: np.ndarray, g2_beta_h: np.ndarray, pub_inputs_list, proofs, ext_msgs=None,
                       on_device: bool = False) -> bool:
    """One pairing product for all proofs.  on_device: the group arithmetic (two MSMs over ~35 terms per proof) runs on
    the GPU through the prover's MSM kernels (capgpu_plonk_batch_verify_dev; needs init()), otherwise on host threads."""
    cnt = len(proofs)
    vk_arr = (ctypes.POINTER(VerifyingKey) * cnt)(*[ctypes.pointer(v) for v in vks])
    pubs = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in pub_inputs_list]
    pub_arr = (u64p * cnt)(*[(_p(p) if p.size else None) for p in pubs])
    nin = (ctypes.c_size_t * cnt)(*[p.size // 4 for p in pubs])
    pr_arr = (ctypes.POINTER(Proof) * cnt)(*[ctypes.pointer(p) for p in proofs])
    msgs = [(m if m is not None else b"") for m in (ext_msgs or [None] * cnt)]
    bufs = [(ctypes.c_uint8 * max(len(m), 1)).from_buffer_copy(m + (b"\0" if not m else b"")) for m in msgs]
    msg_arr = (ctypes.POINTER(ctypes.c_uint8) * cnt)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    len_arr = (ctypes.c_size_t * cnt)(*[len(m) for m in msgs])
    ok = ctypes.c_int(0)
    fn = load().capgpu_plonk_batch_verify_dev if on_device else load().capgpu_plonk_batch_verify
    check(fn(vk_arr, _p(np.ascontiguousarray(g2_h, dtype=np.uint64)),
             _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64)), pub_arr, nin, pr_arr,
             msg_arr, len_arr, ctypes.c_size_t(cnt), ctypes.byref(ok)))
    return bool(ok.value)


# ---- per-proof verification on the device (needs init()) ------------------------------------------------------
def pairing_check_pairs_dev(p: np.ndarray, r: np.ndarray, q1: np.ndarray, q2: np.ndarray) -> np.ndarray:
    """ok[i] = (e(p[i], q1) e(r[i], q2) == 1), one check per GPU lane; p, r: (count, 8) affine G1 words (all-zero =
    infinity), q1, q2: 16-word twist points."""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8)
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 8)
    if p.shape != r.shape:
        raise ValueError("pairing_check_pairs_dev: p and r must hold the same number of points")
    cnt = p.shape[0]
    ok = np.zeros(max(cnt, 1), dtype=np.int32)
    check(load().capgpu_pairing_check_pairs_dev(_p(p.reshape(-1)) if cnt else None, _p(r.reshape(-1)) if cnt else None,
                                                ctypes.c_size_t(cnt), _p(np.ascontiguousarray(q1, dtype=np.uint64)),
                                                _p(np.ascontiguousarray(q2, dtype=np.uint64)),
                                                ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return ok[:cnt] != 0


def plonk_verify_each(vks, g2_h: np.ndarray, g2_beta_h: np.ndarray, pub_inputs_list, proofs,
                      ext_msgs=None) -> np.ndarray:
    """One verdict per proof (capgpu_plonk_verify_each_dev): ok[i] == plonk_verify(vks[i], ..., proofs[i]).  The group
    arithmetic and the pairing check of every proof run on the GPU: finds the bad proofs of a batch that
    plonk_batch_verify rejected."""
    cnt = len(proofs)
    n = max(cnt, 1)
    vk_arr = (ctypes.POINTER(VerifyingKey) * n)(*[ctypes.pointer(v) for v in vks])
    pubs = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in pub_inputs_list]
    pub_arr = (u64p * n)(*[(_p(p) if p.size else None) for p in pubs])
    nin = (ctypes.c_size_t * n)(*[p.size // 4 for p in pubs])
    pr_arr = (ctypes.POINTER(Proof) * n)(*[ctypes.pointer(p) for p in proofs])
    msgs = [(m if m is not None else b"") for m in (ext_msgs or [None] * cnt)]
    bufs = [(ctypes.c_uint8 * max(len(m), 1)).from_buffer_copy(m + (b"\0" if not m else b"")) for m in msgs]
    msg_arr = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
    len_arr = (ctypes.c_size_t * n)(*[len(m) for m in msgs])
    ok = np.zeros(n, dtype=np.int32)
    check(load().capgpu_plonk_verify_each_dev(vk_arr, _p(np.ascontiguousarray(g2_h, dtype=np.uint64)),
                                              _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64)), pub_arr, nin,
                                              pr_arr, msg_arr, len_arr, ctypes.c_size_t(cnt),
                                              ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return ok[:cnt] != 0


PAIRING_LANE, PAIRING_WAVE = 0, 1


def pairing_set_form(form: int) -> None:
    """Which kernel decides the device pairing checks from now on, process-wide (capgpu_pairing_set_form): PAIRING_LANE,
    one check per lane (the default; the environment's CAPGPU_PAIRING=lane|wave sets the initial value), or PAIRING_WAVE,
    one check per group of six lanes - meant for one proof or a small block, not yet timed against LANE.  Callable before init()."""
    check(load().capgpu_pairing_set_form(ctypes.c_int(form)))


def pairing_get_form() -> int:
    form = ctypes.c_int(-1)
    check(load().capgpu_pairing_get_form(ctypes.byref(form)))
    return form.value


def pairing_stats() -> dict:
    """checks decided since process start by each of the two kernels (capgpu_pairing_stats)"""
    lane, wave = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_pairing_stats(ctypes.byref(lane), ctypes.byref(wave)))
    return {"lane_checks": lane.value, "wave_checks": wave.value}


def plonk_verify_dev(vk: VerifyingKey, g2_h: np.ndarray, g2_beta_h: np.ndarray, pub_inputs: np.ndarray, proof: Proof,
                     ext_msg: bytes | None = None) -> bool:
    """plonk_verify with the proof's group arithmetic and its pairing check on the GPU (capgpu_plonk_verify_dev; needs
    init()): same verdict, same errors, the check always in the wave form."""
    pub_inputs = np.ascontiguousarray(pub_inputs, dtype=np.uint64).reshape(-1)
    mbuf, mlen = _bytes_arg(ext_msg)
    ok = ctypes.c_int(0)
    check(load().capgpu_plonk_verify_dev(ctypes.byref(vk), _p(np.ascontiguousarray(g2_h, dtype=np.uint64)),
                                         _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64)),
                                         _p(pub_inputs) if pub_inputs.size else None,
                                         ctypes.c_size_t(pub_inputs.size // 4), mbuf, ctypes.c_size_t(mlen),
                                         ctypes.byref(proof), ctypes.byref(ok)))
    return bool(ok.value)


# ---- the block verifier (capgpu_plonk_verify_block_*; needs init()) ------------------------------------------------------
def plonk_vk_upload(vk: VerifyingKey) -> int:
    """Checks a verifying key once and keeps it for plonk_verify_block (capgpu_plonk_vk_upload) -> handle"""
    h = ctypes.c_uint64(0)
    check(load().capgpu_plonk_vk_upload(ctypes.byref(vk), ctypes.byref(h)))
    return h.value


def plonk_vk_release(vk_handle: int):
    check(load().capgpu_plonk_vk_release(ctypes.c_uint64(vk_handle)))


def _block_msgs(ext_msgs, count: int):
    """ext_msgs / ext_msg_lens of a block call (None, None for no messages) and the buffers they point into"""
    msgs_arg = lens_arg = None
    keep = []
    if ext_msgs is not None and count:
        if len(ext_msgs) != count:
            raise ValueError("plonk_verify_block: one message per proof")
        msgs_arg = (ctypes.POINTER(ctypes.c_uint8) * count)()
        lens_arg = (ctypes.c_size_t * count)()
        for i, m in enumerate(ext_msgs):
            m = bytes(m) if m else b""
            keep.append((ctypes.c_uint8 * max(len(m), 1)).from_buffer_copy(m or b"\0"))
            msgs_arg[i] = ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_uint8))
            lens_arg[i] = len(m)
    return msgs_arg, lens_arg, keep


def plonk_verify_block(vk_handles, g2_h: np.ndarray, g2_beta_h: np.ndarray, pub_rows, proofs, ext_msgs=None,
                       each: bool = False, num_inputs: int | None = None):
    """A whole block decided on the device with one host wait.  vk_handles[i]: proof i's uploaded key; pub_rows: (count,
    num_inputs, 4) array in plonk_prove_multi's layout (a key with fewer inputs uses the first of its row) or a DevBuf of
    that content; proofs: a list of Proof / a (Proof * count) array, or a DevBuf holding the contiguous array - the resident
    entry point is taken when both are DevBufs (then num_inputs must be given).  Returns block_ok, or (block_ok, each_ok)
    with each=True: each_ok[i] == plonk_verify(...) of proof i and block_ok == all(each_ok)."""
    count = len(vk_handles)
    handles = (ctypes.c_uint64 * max(count, 1))(*vk_handles)
    msgs_arg, lens_arg, keep = _block_msgs(ext_msgs, count)
    block_ok = ctypes.c_int(0)
    each_ok = np.zeros(max(count, 1), dtype=np.int32)
    each_arg = each_ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if each else None
    h2 = _p(np.ascontiguousarray(g2_h, dtype=np.uint64))
    bh = _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64))
    if isinstance(proofs, DevBuf) != isinstance(pub_rows, DevBuf):
        raise ValueError("plonk_verify_block: proofs and pub_rows must both be host data or both DevBufs")
    if isinstance(proofs, DevBuf):
        if num_inputs is None or proofs.nbytes < count * ctypes.sizeof(Proof) or pub_rows.nbytes < count * num_inputs * 32:
            raise ValueError("plonk_verify_block: resident buffers need num_inputs and room for count proofs and rows")
        check(load().capgpu_plonk_verify_block_resident(handles, h2, bh, pub_rows.ptr, ctypes.c_size_t(num_inputs),
                                                        proofs.ptr, msgs_arg, lens_arg, ctypes.c_size_t(count),
                                                        ctypes.byref(block_ok), each_arg))
    else:
        pub_rows = np.ascontiguousarray(pub_rows, dtype=np.uint64).reshape(-1)
        if num_inputs is None:
            num_inputs = pub_rows.size // (4 * count) if count else 0
        if pub_rows.size != count * num_inputs * 4:
            raise ValueError(f"plonk_verify_block: pub_rows must hold {count} x {num_inputs} elements")
        if not isinstance(proofs, ctypes.Array):
            arr = (Proof * max(count, 1))()
            for i, pr in enumerate(proofs):
                ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(pr), ctypes.sizeof(Proof))
            proofs = arr
        check(load().capgpu_plonk_verify_block_dev(handles, h2, bh, _p(pub_rows) if pub_rows.size else None,
                                                   ctypes.c_size_t(num_inputs), proofs, msgs_arg, lens_arg,
                                                   ctypes.c_size_t(count), ctypes.byref(block_ok), each_arg))
    if each:
        return bool(block_ok.value), each_ok[:count] != 0
    return bool(block_ok.value)


def verify_sync_stats() -> dict:
    """block-verifier calls that reached the device, and the host waits on the stream they made (capgpu_verify_sync_stats)"""
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(load().capgpu_verify_sync_stats(ctypes.byref(a), ctypes.byref(b)))
    return {"block_calls": a.value, "stream_waits": b.value}


def proof_serialize(proof: Proof) -> bytes:
    buf = (ctypes.c_uint8 * 1024)()
    n = ctypes.c_size_t(0)
    check(load().capgpu_proof_serialize(ctypes.byref(proof), buf, ctypes.c_size_t(1024), ctypes.byref(n)))
    return bytes(buf[:n.value])


def proof_deserialize(data: bytes):
    """-> (Proof, bytes consumed); raises CapGpuError(CAPGPU_ERR_SERIALIZATION) on a malformed encoding."""
    pr, used = Proof(), ctypes.c_size_t(0)
    buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    check(load().capgpu_proof_deserialize(buf, ctypes.c_size_t(len(data)), ctypes.byref(pr), ctypes.byref(used)))
    return pr, used.value


# ---- proofs as note bytes, in bulk and on the device (capgpu_proof_*_batch, capgpu_plonk_verify_block_bytes) -------------
PROOF_BYTES = 769


def _record_array(data, stride: int, count: int | None):
    """bytes / bytearray / np.uint8 array of records `stride` apart -> (contiguous np.uint8 array, count)"""
    if stride < PROOF_BYTES:
        raise ValueError(f"a proof record has {PROOF_BYTES} bytes: stride {stride} is too small")
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview))
                             else np.asarray(data, dtype=np.uint8)).reshape(-1)
    if count is None:
        count = 0 if a.size < PROOF_BYTES else (a.size - PROOF_BYTES) // stride + 1
    if count and a.size < (count - 1) * stride + PROOF_BYTES:
        raise ValueError(f"{a.size} bytes do not hold {count} records {stride} bytes apart")
    return a, count


def _u8p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if a.size else None


def proof_decode_batch(data, count: int | None = None, stride: int = PROOF_BYTES):
    """Bulk Proof::deserialize on the device (capgpu_proof_decode_batch[_dev]).  data: the records as bytes / an np.uint8
    array (count defaults to what they hold) -> ((Proof * count) array, status int32 array), after one wait; or a DevBuf
    (count required) -> (DevBuf of count Proof structs, DevBuf of count ints), enqueued without a wait.  status[i] is 0
    for a record proof_deserialize accepts, else 1 + the byte offset of the first malformed field; such a record decodes
    to all-ones words.  A malformed record never raises."""
    if isinstance(data, DevBuf):
        if count is None or stride < PROOF_BYTES or (count and data.nbytes < (count - 1) * stride + PROOF_BYTES):
            raise ValueError("proof_decode_batch: a DevBuf needs count, stride >= 769 and room for count records")
        d_proofs, d_status = DevBuf(max(count, 1) * ctypes.sizeof(Proof)), DevBuf(max(count, 1) * 4)
        check(load().capgpu_proof_decode_batch_dev(data.ptr, ctypes.c_size_t(stride), ctypes.c_size_t(count), d_proofs.ptr,
                                                   d_status.ptr))
        return d_proofs, d_status
    a, count = _record_array(data, stride, count)
    proofs = (Proof * max(count, 1))()
    status = np.zeros(max(count, 1), dtype=np.int32)
    check(load().capgpu_proof_decode_batch(_u8p(a), ctypes.c_size_t(stride), ctypes.c_size_t(count), proofs,
                                           status.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return proofs, status[:count]


def proof_encode_batch(proofs, count: int | None = None, stride: int = PROOF_BYTES):
    """Bulk capgpu_proof_serialize on the device (capgpu_proof_encode_batch[_dev]).  proofs: a list of Proof / a
    (Proof * count) array -> bytes of (count - 1) * stride + 769 (zero between the records), after one wait; or a DevBuf
    of count contiguous structs (count required) -> a DevBuf of those bytes, enqueued without a wait."""
    if stride < PROOF_BYTES:
        raise ValueError(f"a proof record has {PROOF_BYTES} bytes: stride {stride} is too small")
    if isinstance(proofs, DevBuf):
        if count is None or proofs.nbytes < count * ctypes.sizeof(Proof):
            raise ValueError("proof_encode_batch: a DevBuf needs count and room for count proofs")
        d_bytes = DevBuf((count - 1) * stride + PROOF_BYTES if count else 1)
        check(load().capgpu_proof_encode_batch_dev(proofs.ptr, ctypes.c_size_t(count), d_bytes.ptr, ctypes.c_size_t(stride)))
        return d_bytes
    count = len(proofs) if count is None else count
    if not isinstance(proofs, ctypes.Array):
        arr = (Proof * max(count, 1))()
        for i, pr in enumerate(proofs):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(pr), ctypes.sizeof(Proof))
        proofs = arr
    out = np.zeros((count - 1) * stride + PROOF_BYTES if count else 0, dtype=np.uint8)
    check(load().capgpu_proof_encode_batch(proofs, ctypes.c_size_t(count), _u8p(out), ctypes.c_size_t(stride)))
    return out.tobytes()


def plonk_verify_block_bytes(vk_handles, g2_h: np.ndarray, g2_beta_h: np.ndarray, pub_rows, proof_bytes, ext_msgs=None,
                             each: bool = False, num_inputs: int | None = None, stride: int = PROOF_BYTES,
                             status: bool = False):
    """plonk_verify_block with the proofs as their 769 note bytes, `stride` apart: bytes / an np.uint8 array with pub_rows
    an array, or both DevBufs (capgpu_plonk_verify_block_bytes / _bytes_resident; then num_inputs must be given).  The
    records are decoded on the device in front of the block verifier's launches, inside its one wait.  Returns block_ok,
    (block_ok, each_ok) with each=True, and the decode statuses (proof_decode_batch's) as a last element with status=True:
    each_ok[i] == (status[i] == 0 and plonk_verify(...) of the decoded proof), block_ok == all(each_ok)."""
    count = len(vk_handles)
    handles = (ctypes.c_uint64 * max(count, 1))(*vk_handles)
    msgs_arg, lens_arg, keep = _block_msgs(ext_msgs, count)
    block_ok = ctypes.c_int(0)
    each_ok = np.zeros(max(count, 1), dtype=np.int32)
    st = np.zeros(max(count, 1), dtype=np.int32)
    each_arg = each_ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if each else None
    st_arg = st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if status else None
    h2 = _p(np.ascontiguousarray(g2_h, dtype=np.uint64))
    bh = _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64))
    if isinstance(proof_bytes, DevBuf) != isinstance(pub_rows, DevBuf):
        raise ValueError("plonk_verify_block_bytes: proof_bytes and pub_rows must both be host data or both DevBufs")
    if isinstance(proof_bytes, DevBuf):
        if num_inputs is None or stride < PROOF_BYTES or pub_rows.nbytes < count * num_inputs * 32 or \
                (count and proof_bytes.nbytes < (count - 1) * stride + PROOF_BYTES):
            raise ValueError("plonk_verify_block_bytes: resident buffers need num_inputs and room for count records and rows")
        check(load().capgpu_plonk_verify_block_bytes_resident(handles, h2, bh, pub_rows.ptr, ctypes.c_size_t(num_inputs),
                                                              proof_bytes.ptr, ctypes.c_size_t(stride), msgs_arg, lens_arg,
                                                              ctypes.c_size_t(count), ctypes.byref(block_ok), each_arg,
                                                              st_arg))
    else:
        pub_rows = np.ascontiguousarray(pub_rows, dtype=np.uint64).reshape(-1)
        if num_inputs is None:
            num_inputs = pub_rows.size // (4 * count) if count else 0
        if pub_rows.size != count * num_inputs * 4:
            raise ValueError(f"plonk_verify_block_bytes: pub_rows must hold {count} x {num_inputs} elements")
        a, _ = _record_array(proof_bytes, stride, count)
        check(load().capgpu_plonk_verify_block_bytes(handles, h2, bh, _p(pub_rows) if pub_rows.size else None,
                                                     ctypes.c_size_t(num_inputs), _u8p(a), ctypes.c_size_t(stride), msgs_arg,
                                                     lens_arg, ctypes.c_size_t(count), ctypes.byref(block_ok), each_arg,
                                                     st_arg))
    out = (bool(block_ok.value),) + ((each_ok[:count] != 0,) if each else ()) + ((st[:count],) if status else ())
    return out[0] if len(out) == 1 else out


# ---- on-disk parameter formats (include/capgpu.h) ----------------------------------------
CAPGPU_ERR_SERIALIZATION = -8


def _u8buf(b: bytes):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def _opt_words(a, n):
    return _p(np.ascontiguousarray(a, dtype=np.uint64).reshape(n)) if a is not None else None


def g1_decompress(data: bytes) -> np.ndarray:
    """n x 32 bytes -> (n, 8) affine Montgomery words, (0, 0) = infinity."""
    n = len(data) // 32
    out = np.zeros((n, 8), dtype=np.uint64)
    check(load().capgpu_g1_decompress(_u8buf(data), ctypes.c_size_t(n), _p(out.reshape(-1)) if n else None))
    return out


def g1_compress(points: np.ndarray) -> bytes:
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n = points.shape[0]
    out = (ctypes.c_uint8 * max(32 * n, 1))()
    check(load().capgpu_g1_compress(_p(points.reshape(-1)) if n else None, ctypes.c_size_t(n), out))
    return bytes(out[:32 * n])


def srs_deserialize(data: bytes, max_degree: int = 0):
    """-> (handle, h, beta_h, consumed)"""
    handle, used = ctypes.c_uint64(0), ctypes.c_size_t(0)
    h, bh = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    check(load().capgpu_srs_deserialize(_u8buf(data), ctypes.c_size_t(len(data)), ctypes.c_size_t(max_degree),
                                        ctypes.byref(handle), _p(h), _p(bh), ctypes.byref(used)))
    return handle.value, h, bh, used.value


def _sized_call(fn, *head):
    n = ctypes.c_size_t(0)
    check(fn(*head, None, ctypes.c_size_t(0), ctypes.byref(n)))
    buf = (ctypes.c_uint8 * max(n.value, 1))()
    check(fn(*head, buf, ctypes.c_size_t(n.value), ctypes.byref(n)))
    return bytes(buf[:n.value])


def srs_serialize(handle: int, h: np.ndarray, beta_h: np.ndarray) -> bytes:
    return _sized_call(load().capgpu_srs_serialize, ctypes.c_uint64(handle), _opt_words(h, 16), _opt_words(beta_h, 16))


def plonk_vk_serialize(vk: VerifyingKey, g: np.ndarray, h: np.ndarray, beta_h: np.ndarray, gamma_g=None) -> bytes:
    return _sized_call(load().capgpu_plonk_vk_serialize, ctypes.byref(vk), _opt_words(g, 8), _opt_words(gamma_g, 8),
                       _opt_words(h, 16), _opt_words(beta_h, 16))


def plonk_vk_deserialize(data: bytes):
    """-> (vk, g, gamma_g, h, beta_h, consumed)"""
    vk, used = VerifyingKey(), ctypes.c_size_t(0)
    g, gg = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    h, bh = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    check(load().capgpu_plonk_vk_deserialize(_u8buf(data), ctypes.c_size_t(len(data)), ctypes.byref(vk), _p(g), _p(gg),
                                             _p(h), _p(bh), ctypes.byref(used)))
    return vk, g, gg, h, bh, used.value


def plonk_key_serialize(pk_handle: int, h: np.ndarray, beta_h: np.ndarray, gamma_g=None) -> bytes:
    return _sized_call(load().capgpu_plonk_key_serialize, ctypes.c_uint64(pk_handle), _opt_words(gamma_g, 8),
                       _opt_words(h, 16), _opt_words(beta_h, 16))


def plonk_key_deserialize(data: bytes):
    """-> (srs_handle, pk_handle, vk, h, beta_h, consumed)"""
    srs, pk, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_size_t(0)
    vk = VerifyingKey()
    h, bh = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    check(load().capgpu_plonk_key_deserialize(_u8buf(data), ctypes.c_size_t(len(data)), ctypes.byref(srs),
                                              ctypes.byref(pk), ctypes.byref(vk), _p(h), _p(bh), ctypes.byref(used)))
    return srs.value, pk.value, vk, h, bh, used.value


# ---- parameter audit (needs init()) ----------------------------------------------------------------------------
SRS_CHECK_LOCATE = 1


class SrsReport(ctypes.Structure):
    """capgpu_srs_report (include/capgpu.h): the verdict of capgpu_srs_check."""
    _fields_ = [
        ("verdict", ctypes.c_uint32),           # 0 consistent, 1 point fault, 2 structure fault
        ("point_fault", ctypes.c_uint32),       # 0 none, 1 a point at infinity, 2 a point off the curve
        ("first_bad_point", ctypes.c_uint64),
        ("first_bad_link", ctypes.c_uint64),
        ("points_checked", ctypes.c_uint64),
        ("links_checked", ctypes.c_uint64),
        ("pairing_checks", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("fold_a", ctypes.c_uint64 * 8),
        ("fold_b", ctypes.c_uint64 * 8),
    ]

    def __str__(self):
        """'' for a consistent SRS, else the fault in words"""
        if self.verdict == 1:
            what = "is the point at infinity" if self.point_fault == 1 else "is not on the curve"
            return f"SRS point {self.first_bad_point} {what}"
        if self.verdict == 2:
            where = "" if self.first_bad_link == 2**64 - 1 else \
                f"; first bad link: point {self.first_bad_link + 1} is not tau times point {self.first_bad_link}"
            return "SRS is not a power sequence under the open key" + where
        return ""


class KeyReport(ctypes.Structure):
    """capgpu_key_report (include/capgpu.h): the verdict of capgpu_plonk_key_check."""
    _fields_ = [
        ("verdict", ctypes.c_uint32),   # 0 consistent, 1 shape, 2 commitment differs, 3 sigma is no permutation
        ("column", ctypes.c_uint32),    # verdict 2: 0..12 selector, 13..17 sigma; the lowest differing
        ("columns_differing", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]

    def __str__(self):
        if self.verdict == 1:
            return "proving key and verifying key differ in domain_size, num_inputs or k"
        if self.verdict == 2:
            col = f"selector {self.column}" if self.column < NUM_SELECTORS else f"sigma {self.column - NUM_SELECTORS}"
            return (f"the proving key's polynomials do not commit to the verifying key: {self.columns_differing} of 18 "
                    f"commitments differ, first: {col}")
        if self.verdict == 3:
            return "sigma is not a permutation of the extended domain"
        return ""


def srs_check(handle: int, g2_h: np.ndarray, g2_beta_h: np.ndarray, seed: bytes | None = None,
              locate: bool = False) -> SrsReport:
    """Is the resident SRS [tau^i] g for the tau of the open key (h, beta_h)?  The report holds the verdict; seed: 32
    bytes for a reproducible check, None to draw them from the OS.  Call once per loaded file, not per proof."""
    if seed is not None and len(seed) != 32:
        raise ValueError("srs_check: the seed is 32 bytes")
    rep = SrsReport()
    check(load().capgpu_srs_check(ctypes.c_uint64(handle), _p(np.ascontiguousarray(g2_h, dtype=np.uint64)),
                                  _p(np.ascontiguousarray(g2_beta_h, dtype=np.uint64)),
                                  _u8buf(seed) if seed is not None else None,
                                  ctypes.c_uint32(SRS_CHECK_LOCATE if locate else 0), ctypes.byref(rep)))
    return rep


def plonk_key_check(pk_handle: int, vk: VerifyingKey | None = None) -> KeyReport:
    """Does the proving key commit to this verifying key (None: the key's own, e.g. the one its blob carried)?"""
    rep = KeyReport()
    check(load().capgpu_plonk_key_check(ctypes.c_uint64(pk_handle), ctypes.byref(vk) if vk is not None else None,
                                        ctypes.byref(rep)))
    return rep
