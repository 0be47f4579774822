"""The argument checks of the proving and witness-check entry points at the C boundary, on the device: for every entry
point the (return code, text of capgpu_last_error) of each refusal, the order in which the refusals take precedence, and
one accepted call whose proofs are word for word the lone capgpu_plonk_prove's.  The symbols are called through ctypes
directly (tests/test_prove_each_abi.py does the same without a device); the codes and texts are literals taken from the
library's source, so that a change of the code behind the boundary cannot move them unnoticed.

Circuits of n = 16 (synthetic_circuit(4, 1) and (4, 0)), batches of 3: every case takes milliseconds.

One refusal of the library has no case here: "rows of %zu variables given, the key of proof %u has %zu" cannot be provoked
through the C boundary, which takes no row length - it derives the stride of a variable-form call from the call's own keys
(the largest num_vars among them).  The variable-form positive cases use two keys of DIFFERENT num_vars instead, so that
one key's rows are longer than its own table needs."""
import ctypes

import numpy as np
import pytest

from cap_amd import bench_utils as bu
from tests.test_gpu_vars_prove import var_values

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, BAD_HANDLE = 0, -1, -4
UNKNOWN = 999999  # a handle the library never issued

PROVE = "capgpu_plonk_prove"
BATCH = ("batch_ex", "batch_dev_ex", "batch_async")
MULTI = ("multi_ex", "multi_dev_ex", "multi_async")
EACH = ("each", "each_dev", "each_async")
LONE = ("prove_ex", "prove_ex+co")  # capgpu_plonk_prove_ex without and with coalescing
CHECK1 = ("check_witness", "check_witness_batch", "check_witness_batch_dev")
CHECK = CHECK1 + ("check_witness_multi",)
PROVING = BATCH + MULTI + EACH
ALL = PROVING + LONE + CHECK
PER_PROOF_KEYS = MULTI + EACH + ("check_witness_multi",)  # a handle per proof
COUNTED = tuple(n for n in ALL if n not in LONE + ("check_witness",))  # take a `count`

BAD = {**{n: "capgpu_plonk_prove: bad argument" for n in BATCH + LONE},
       **{n: "capgpu_plonk_prove_multi: bad argument" for n in MULTI + EACH},
       **{n: "capgpu_plonk_check_witness: bad argument" for n in CHECK1},
       "check_witness_multi": "capgpu_plonk_check_witness_multi: bad argument"}
FORM7 = "capgpu_plonk: input_form 7 is none of CAPGPU_INPUT_EVALS (0), CAPGPU_INPUT_COEFFS (1), CAPGPU_INPUT_VARS (2)"
UNKNOWN_KEY = "capgpu: unknown proving key handle 999999"
NO_TABLE = "capgpu_plonk: CAPGPU_INPUT_VARS: key has no variable table"
SHARE = "capgpu_plonk_prove_multi: the keys of one batch must share the domain size and the SRS"
SHARE_CHECK = "capgpu_plonk_check_witness_multi: the keys of one batch must share the domain size and the SRS"
# the pointers each entry point refuses when NULL (p: the public inputs, with num_inputs = 1)
POINTERS = {**{n: "wpbr" for n in ("batch_ex", "batch_dev_ex") + LONE}, "batch_async": "wpbrt",
            "multi_ex": "hwpbr", "multi_dev_ex": "hwpbr", "multi_async": "hwpbrt",
            "each": "hwpbro", "each_dev": "hwpbro", "each_async": "hwpbrot",
            **{n: "wpf" for n in CHECK1}, "check_witness_multi": "hwpf"}


def symbol(name):
    if name in CHECK:
        return "capgpu_plonk_" + name
    if name in LONE:
        return "capgpu_plonk_prove_ex"
    return "capgpu_plonk_prove_" + name


class Result:
    def __init__(self, rc, err, proofs, outcomes, faults, ticket, waited):
        self.rc, self.err, self.proofs, self.outcomes, self.faults = rc, err, proofs, outcomes, faults
        self.ticket, self.waited = ticket, waited  # waited: capgpu_wait's return code, None when nothing was queued


def call(cg, name, a, null="", **over):
    """One call of entry point `name` with the arguments of dict `a` (h: handles, count, w: wires, p: public inputs, nin,
    m: one message or a list of them, b: blinders, form), `over` replacing some, the pointers named in `null` NULL
    (h w p b r(proofs) o(utcomes) f(aults) t(icket) l(engths of the messages))."""
    L = cg.load()
    a = {**a, **over}
    count, k = a["count"], max(a["count"], 1)
    arr = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)        # noqa: E731
    handles = (ctypes.c_uint64 * k)(*a["h"][:k])
    key = handles if name in PER_PROOF_KEYS else ctypes.c_uint64(a["h"][0])
    if "h" in null:
        key = None
    w = arr(a["w"])
    dbuf = cg.DevBuf.from_numpy(w) if "_dev" in name else None
    wires = None if "w" in null else (dbuf.ptr if dbuf else cg._p(w))
    pubs = arr(a["p"]) if a["p"] is not None else None
    pub_ptr = None if ("p" in null or pubs is None or not pubs.size) else cg._p(pubs)
    nin = ctypes.c_size_t(a["nin"])
    form = ctypes.c_int(a["form"])
    proofs, outcomes, faults = (cg.Proof * k)(), (cg.ProveOutcome * k)(), (cg.WitnessFault * k)()
    ticket = ctypes.c_uint64(7)
    rc = waited = None
    if name in CHECK:
        f = None if "f" in null else faults
        head = [key] + ([count] if name != "check_witness" else [])
        rc = getattr(L, symbol(name))(*head, wires, pub_ptr, nin, form, f)
    else:
        bl = arr(a["b"])
        tail = [None if "b" in null else cg._p(bl), form, None if "r" in null else proofs]
        if name in BATCH + LONE:
            m = a["m"]
            msg = [(ctypes.c_uint8 * len(m)).from_buffer_copy(m) if m else None, ctypes.c_size_t(len(m) if m else 0)]
            head = [key] + ([count] if name in BATCH else [])
        else:
            msg = [None, None]
            if a["m"] is not None:
                keep = [bytes(x) if x else None for x in a["m"]]
                msg = [(ctypes.c_char_p * k)(*keep[:k]),
                       None if "l" in null else (ctypes.c_size_t * k)(*[len(x) if x else 0 for x in keep[:k]])]
            head = [key, count]
        if name in EACH:
            tail.append(None if "o" in null else outcomes)
        if name.endswith("_async"):
            tail.append(None if "t" in null else ctypes.byref(ticket))
        if name == "prove_ex+co":
            cg.plonk_set_coalescing(200, 0)
        try:
            rc = getattr(L, symbol(name))(*head, wires, pub_ptr, nin, *msg, *tail)
        finally:
            if name == "prove_ex+co":
                cg.plonk_set_coalescing(0, 0)
    err = L.capgpu_last_error().decode() if rc else ""
    if name.endswith("_async") and rc == OK and "t" not in null and ticket.value:
        done = ctypes.c_int(0)
        waited = L.capgpu_wait(ticket, ctypes.c_uint32(0xFFFFFFFF), ctypes.byref(done))
        assert done.value == 1
        if waited:
            err = L.capgpu_last_error().decode()
    if dbuf:
        dbuf.free()
    return Result(rc, err, proofs, outcomes, faults, ticket.value, waited)


def refused(cg, name, a, code, text, **kw):
    r = call(cg, name, a, **kw)
    print(name, kw, "->", r.rc, repr(r.err))
    assert r.rc == code and text in r.err, f"{name} {kw}: got ({r.rc}, {r.err!r}), want ({code}, ...{text!r}...)"
    assert r.waited is None  # an argument error is the submitting call's, never the ticket's


class World:
    """two SRS, the keys, three witnesses in both forms under two keys and under one, and every lone proof"""

    def __init__(self, cg, tau):
        self.cg = cg
        scA, scB, sc32 = bu.synthetic_circuit(4, 1, seed=5), bu.synthetic_circuit(4, 0, seed=4), bu.synthetic_circuit(5, 1)
        self.srs = [cg.srs_generate(tau, 32 + 3), cg.srs_generate(tau + 1, 16 + 3)]
        nvA, nvB = scA.num_vars, scB.num_vars + 5
        assert nvA != nvB
        pre = lambda h, sc: cg.plonk_preprocess(h, sc.n, sc.num_inputs, sc.selectors_mont(), sc.sigma_mont())[0]  # noqa: E731
        prv = lambda sc, nv: cg.plonk_preprocess_vars(self.srs[0], sc.n, sc.num_inputs, sc.selectors_mont(),  # noqa: E731
                                                      np.array(sc.wire_vars), nv)[0]
        self.kA, self.kB = prv(scA, nvA), prv(scB, nvB)                        # keys with a variable table
        self.plain = pre(self.srs[0], scA)                                   # the circuit of kA, no table
        self.other_srs, self.n32 = pre(self.srs[1], scA), pre(self.srs[0], sc32)
        self.keys = [self.kA, self.kB, self.plain, self.other_srs, self.n32]

        def batch(order, seeds):
            nvs = [nvA if sc is scA else nvB for sc in order]
            # variable form: rows of the largest num_vars among the call's keys
            W, V, Pb, Bl = [], np.zeros((3, max(nvs), 4), np.uint64), np.zeros((3, 1, 4), np.uint64), []
            V[:] = bu.to_mont_array([12345])[0]  # what lies behind a shorter key's values must not matter
            for i, (sc, nv, s) in enumerate(zip(order, nvs, seeds)):
                w, pubs = sc.witness(s)
                W.append(sc.wires_mont(w))
                V[i, :nv] = var_values(sc, w, nv, s)
                if pubs:
                    Pb[i] = bu.to_mont_array(pubs)
                Bl.append(bu.to_mont_array(bu.blinders(700 + s)))
            return np.stack(W), V, Pb, np.stack(Bl)

        msgs = [b"note-0", None, b"note-2"]
        W2, V2, P2, B2 = batch([scA, scB, scA], [11, 12, 13])
        W1, V1, P1, B1 = batch([scA, scA, scA], [11, 14, 13])
        two = dict(h=[self.kA, self.kB, self.kA], count=3, p=P2, nin=1, m=msgs, b=B2)
        one = dict(h=[self.kA] * 3, count=3, p=P1, nin=1, m=msgs, b=B1)
        # args[(keys, form)]: "two" - three proofs under two keys, "one" - under one key with a message per proof,
        # "memo" - under one key with one shared message (the capgpu_plonk_prove_batch* family)
        self.args = {("two", 0): dict(two, w=W2, form=0), ("two", 2): dict(two, w=V2, form=2),
                     ("one", 0): dict(one, w=W1, form=0), ("one", 2): dict(one, w=V1, form=2),
                     ("memo", 0): dict(one, w=W1, form=0, m=b"memo"), ("memo", 2): dict(one, w=V1, form=2, m=b"memo")}

        def lone(a, W):  # capgpu_plonk_prove of each witness's columns, with the message the batch gives that proof
            out = []
            for i in range(3):
                m = a["m"] if isinstance(a["m"], bytes) else a["m"][i]
                nin = cg.plonk_key_info(a["h"][i])[1]
                out.append(bytes(cg.plonk_prove(a["h"][i], W[i], a["p"][i][:nin], a["b"][i], m)))
            return out

        self.lone = {"two": lone(two, W2), "one": lone(one, W1), "memo": lone(self.args[("memo", 0)], W1)}

    def of(self, name, form=0):
        """the accepted call of this entry point: (arguments, lone proofs)"""
        if name in LONE or name == "check_witness":  # one proof: the first of the shared-message batch
            a = self.args[("memo", form)]
            return dict(a, count=1, w=a["w"][:1], p=a["p"][:1], b=a["b"][:1]), self.lone["memo"][:1]
        kind = "memo" if name in BATCH + CHECK1 else "two"
        return self.args[(kind, form)], self.lone[kind]

    def free(self):
        for k in self.keys:
            self.cg.plonk_free_key(k)
        for h in self.srs:
            self.cg.srs_free(h)


@pytest.fixture(scope="module")
def world(cg, tau):
    w = World(cg, tau)
    yield w
    w.free()


# ---- accepted calls --------------------------------------------------------------------------------------------------------
def accepted(cg, name, a, want):
    r = call(cg, name, a)
    assert r.rc == OK, (name, r.rc, r.err)
    if name.endswith("_async"):
        assert r.ticket != 0 and r.waited == OK, (name, r.waited, r.err)
    cnt = a["count"]
    if name in CHECK:
        assert [f.kind for f in r.faults[:cnt]] == [0] * cnt
        return
    assert [bytes(p) for p in r.proofs[:cnt]] == want, f"{name}: not the lone calls' proofs"
    if name in EACH:
        assert [(o.status, o.degree_flags, o.fault.kind) for o in r.outcomes[:cnt]] == [(0, 0, 0)] * cnt


@pytest.mark.parametrize("form", [0, 2], ids=["evals", "vars"])
@pytest.mark.parametrize("name", ALL)
def test_accepted_call_gives_the_lone_proofs(cg, world, name, form):
    a, want = world.of(name, form)
    accepted(cg, name, a, want)


@pytest.mark.parametrize("form", [0, 2], ids=["evals", "vars"])
@pytest.mark.parametrize("name", EACH)
def test_outcome_call_of_one_key_gives_each_proof_its_own_message(cg, world, name, form):
    accepted(cg, name, world.args[("one", form)], world.lone["one"])


def test_rows_longer_than_the_keys_need_are_repacked_by_the_synchronous_multi_call(cg, world):
    a, want = world.of("multi_ex")
    wide = np.zeros((3, 2, 4), np.uint64)
    wide[:, :1] = a["p"]
    accepted(cg, "multi_ex", dict(a, p=wide, nin=2), want)
    refused(cg, "multi_async", dict(a, p=wide, nin=2), INVALID_ARG,
            "capgpu_plonk_prove_multi: rows of 2 public inputs given, the keys need 1")


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_null_pointers_bad_count_and_bad_form(cg, world, name):
    a, _ = world.of(name)
    for ptr in POINTERS[name]:
        refused(cg, name, a, INVALID_ARG, BAD[name], null=ptr)
    if name in COUNTED:
        refused(cg, name, a, INVALID_ARG, BAD[name], count=-1)
    refused(cg, name, a, INVALID_ARG, FORM7, form=7)
    if name in MULTI + EACH:
        refused(cg, name, a, INVALID_ARG, BAD[name], null="l")  # messages without their lengths


@pytest.mark.parametrize("name", COUNTED)
def test_empty_batch_is_accepted(cg, world, name):
    a, _ = world.of(name)
    r = call(cg, name, a, count=0)
    assert r.rc == OK and r.waited is None
    if name.endswith("_async"):
        assert r.ticket == 0  # (the call overwrote the 7 it found there)


@pytest.mark.parametrize("name", ALL)
def test_unknown_handle(cg, world, name):
    a, _ = world.of(name)
    refused(cg, name, a, BAD_HANDLE, UNKNOWN_KEY, h=[UNKNOWN] + a["h"][1:])
    if name in PER_PROOF_KEYS:
        refused(cg, name, a, BAD_HANDLE, UNKNOWN_KEY, h=a["h"][:2] + [UNKNOWN])


# An unknown handle together with a NULL blinders (the check calls: faults) pointer.  The host-buffer calls of one key and
# of several keys - synchronous and by ticket - look the first key up BEFORE they look at the remaining pointers; the
# device-buffer calls, the outcome calls and the coalescing capgpu_plonk_prove_ex check every pointer first.
HANDLE_FIRST = ("batch_ex", "batch_async", "multi_ex", "multi_async", "prove_ex")


@pytest.mark.parametrize("name", ALL)
def test_unknown_handle_with_a_null_pointer(cg, world, name):
    a, _ = world.of(name)
    bad = dict(h=[UNKNOWN] + a["h"][1:], null="f" if name in CHECK else "b")
    if name in HANDLE_FIRST:
        refused(cg, name, a, BAD_HANDLE, UNKNOWN_KEY, **bad)
    else:
        refused(cg, name, a, INVALID_ARG, BAD[name], **bad)


@pytest.mark.parametrize("name", ALL)
def test_wrong_num_inputs(cg, world, name):
    a, _ = world.of(name)
    one_key = "0 public inputs given, key expects 1"
    rows = "rows of 0 public inputs given, the keys need 1"
    text = {**{n: "capgpu_plonk_prove: " + one_key for n in BATCH + LONE},
            **{n: "capgpu_plonk_prove_multi: " + rows for n in MULTI + EACH},
            **{n: "capgpu_plonk_check_witness: " + one_key for n in CHECK1},
            "check_witness_multi": "capgpu_plonk_check_witness_multi: " + rows}[name]
    refused(cg, name, a, INVALID_ARG, text, nin=0, p=None)
    if name in EACH:  # handles that all name one key: the single-key call's wording
        refused(cg, name, world.args[("one", 0)], INVALID_ARG, "capgpu_plonk_prove: " + one_key, nin=0, p=None)


@pytest.mark.parametrize("name", PER_PROOF_KEYS)
def test_keys_of_another_domain_size_or_srs(cg, world, name):
    a, _ = world.of(name)
    text = SHARE_CHECK if name in CHECK else SHARE
    refused(cg, name, a, INVALID_ARG, text, h=[world.plain, world.n32, world.plain])
    refused(cg, name, a, INVALID_ARG, text, h=[world.plain, world.other_srs, world.plain])


@pytest.mark.parametrize("name", ALL)
def test_variable_form_with_a_key_that_has_no_table(cg, world, name):
    a, _ = world.of(name, 2)
    refused(cg, name, a, INVALID_ARG, NO_TABLE, h=[world.plain] * 3)
    if name in PER_PROOF_KEYS:
        refused(cg, name, a, INVALID_ARG, NO_TABLE, h=[world.kA, world.plain, world.kA])
