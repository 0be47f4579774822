"""The NTT at every plan: whole outputs through the C ABI (cg.ntt_fr_dev), bit for bit against the C restatement, after
asserting through cg.ntt_plan that the shape reached the plan the case was written for.

What the earlier NTT tests leave out (they total fewer than 2^17 elements per call, which tile_log_for answers with the
256-element tile every time): the 512- and the 1024-element tile (count << log_n = 2^17 and 2^18), tile widths log_c up to
4, the three-pass plan compared in full at both of its digit splits ((7, 7, 7) at 2^21, (8, 7, 7) at 2^22), the
2048-element tile, the fixed 256-element tile on a large launch, and the persistent instantiations of both passes.  The
inputs (tools/ntt_conformance.py: INPUTS) put zeros on either operand of the butterflies' zero shortcuts and limbs at
their maximum; one of them is x + r as the raw image of x.  Padding between arrays is filled with a sentinel and must
come back untouched.

The default environment runs in this process.  The forced environments are read once per process, so each is ONE fresh
child (python -m tools.ntt_conformance ...), one at a time, each under its own time limit; after a child that ended by a
signal, at its limit, with an exception (a HIP error among them) or in any way but a clean 0 or 1, no further child is
started and the remaining cases fail with that reason.

Time limits: five times the child's wall time measured on the MI355X, not below 60 s.  MEASURED_S below holds the
measured wall times per configuration (seconds, on the MI355X, the oracle's transforms included)."""
import json
import os
import subprocess
import sys
import time

import pytest

from tools import ntt_conformance as nc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# digits of each pass in the order they run, as ntt.hip splits log_n (written out here, not computed: a change of the
# split has to show up as a failure of these tests)
DIGITS = {1: [1], 2: [2], 3: [3], 5: [5], 8: [8], 9: [9], 10: [10], 11: [6, 5], 12: [6, 6], 13: [7, 6], 14: [7, 7],
          16: [8, 8], 20: [10, 10], 21: [7, 7, 7], 22: [8, 7, 7]}


def expected_log_c(log_n, tile_log):
    """tile width of each pass: what is left of the tile after the digit, at most 4, and no more than there are columns
    (column pass: the rest of the segment; row pass: the leading digit)"""
    d = DIGITS[log_n]
    out, rest = [], log_n
    for i, dig in enumerate(d):
        rest -= dig
        room = rest if i + 1 < len(d) else (d[0] if len(d) > 1 else 0)
        out.append(max(0, min(tile_log - dig, 4, room)))
    return out


def check_plan(plan, log_n, tile_log, persistent=None):
    d = DIGITS[log_n]
    assert plan["passes"] == len(d) and plan["digits"] == d, plan
    assert plan["tile_log"] == tile_log, plan
    assert plan["log_c"] == expected_log_c(log_n, tile_log), plan
    assert plan["tiles"] == [1 << (log_n - dig - c) for dig, c in zip(d, plan["log_c"])], plan
    assert plan["persistent"] == (persistent if persistent is not None else [False] * len(d)), plan


def count_for(log_n, level):
    """`count` with count << log_n below 2^17 (an odd count where there is room), exactly 2^17, exactly 2^18"""
    if level == 8:
        return (1 << (16 - log_n)) + 1 if log_n < 16 else 1
    return 1 << ({9: 17, 10: 18}[level] - log_n)


SMALL = [(log_n, level) for log_n in (1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 16) for level in (8, 9, 10)]


@pytest.mark.parametrize("log_n,tile_log", SMALL)
def test_whole_outputs_at_each_tile_size(cg, log_n, tile_log):
    """single-pass and two-pass plans at the 256-, 512- and 1024-element tile, all four (dir, coset) pairs"""
    count = count_for(log_n, tile_log)
    total = count << log_n
    assert (total < 1 << 17) if tile_log == 8 else total == 1 << (tile_log + 8)
    check_plan(cg.ntt_plan(log_n, count), log_n, tile_log)
    res = nc.run_shape(cg, log_n, count)
    assert res["arrays"] >= 4 * len(nc.INPUTS)
    assert not res["mismatches"], "\n".join(res["mismatches"])


def test_tile_widths_cover_zero_to_four(cg):
    """the shapes above give log_c every value from 0 to 4 in the column pass and in the row pass"""
    col, row = set(), set()
    for log_n, level in SMALL + [(20, 10)]:
        plan = cg.ntt_plan(log_n, count_for(log_n, level) if log_n < 20 else 1)
        if plan["passes"] == 2:
            col.add(plan["log_c"][0])
        row.add(plan["log_c"][-1])
    assert col == {0, 1, 2, 3, 4} and row == {0, 1, 2, 3, 4}, (col, row)


@pytest.mark.parametrize("inverse,coset", nc.MODES)
@pytest.mark.parametrize("log_n", [20, 21, 22])
def test_large_transforms_in_full(cg, log_n, inverse, coset):
    """count = 1: two passes of 2^10 with log_c = 0, and the three-pass plan at both digit splits - every element of the
    output, not samples (one (dir, coset) pair per case: the oracle's 2^22-point transform takes seconds)"""
    check_plan(cg.ntt_plan(log_n, 1), log_n, 10)
    res = nc.run_shape(cg, log_n, 1, modes=[(inverse, coset)])
    assert res["arrays"] == len(nc.INPUTS)
    assert not res["mismatches"], "\n".join(res["mismatches"])


def test_padding_between_arrays_is_left_alone(cg):
    """stride > n: the padding holds a sentinel (the existing test only has padding that started as zero)"""
    log_n, count, stride = 12, 5, (1 << 12) + 7
    check_plan(cg.ntt_plan(log_n, count), log_n, 8)
    res = nc.run_shape(cg, log_n, count, stride=stride)
    assert res["stride"] == stride and not res["mismatches"], "\n".join(res["mismatches"])


# ---- forced environments: one fresh child each -------------------------------------------------------------------
# name -> (environment, shapes, what check_plan is given per shape: (tile_log, persistent))
CONFIGS = {
    # digits of 7 and more: a tile is at most 2^(digit + 4) elements, so these reach 2048 in the passes whose digit is 7
    # or more (2^14, 2^16 and 2^21: in every pass)
    "tile2048": ({"CAPGPU_NTT_TILE_LOG": "11"}, {"13:64": (11, None), "14:32": (11, None), "16:8": (11, None)}),
    "tile2048_three_pass": ({"CAPGPU_NTT_TILE_LOG": "11"}, {"21:1": (11, None)}),
    "tile256_fixed": ({"CAPGPU_NTT_TILE_LOG": "8", "CAPGPU_NTT_TILE_ADAPT": "0"},
                      {"9:512": (8, None), "12:64": (8, None), "16:4": (8, None)}),
    # 16 tiles per array and pass, 128 arrays: 2048 tiles, above the threshold of 4 * 256 * 1
    "persistent1": ({"CAPGPU_NTT_PERSISTENT": "1", "CAPGPU_NTT_TILE_LOG": "8"}, {"12:128": (8, [True, True])}),
    # 2048 tiles per array and pass: count = 1 sits ON the threshold of 4 * 256 * 2 and is not persistent (its plan alone
    # is asserted: the launch is the one test_large_transforms_in_full compares), count = 2 is above it and runs in full
    "persistent2": ({"CAPGPU_NTT_PERSISTENT": "2"}, {"plan=21:1": (10, [False] * 3), "21:2": (10, [True] * 3)}),
}
MEASURED_S = {"tile2048": 1.4, "tile2048_three_pass": 13.5, "tile256_fixed": 0.9, "persistent1": 0.5, "persistent2": 14.2}
_stopped = []          # the reason no further child is started, once there is one
_results = {}


def time_limit(name):
    return max(60.0, 5 * (MEASURED_S[name] or 0))


def run_config(name):
    if name in _results:
        return _results[name]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env_add, shapes = CONFIGS[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("CAPGPU_NTT_")}
    env.update(env_add)
    t0 = time.time()
    try:
        out = subprocess.run([sys.executable, "-m", "tools.ntt_conformance"] + list(shapes), cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=time_limit(name))
        code, stdout, stderr = out.returncode, out.stdout, out.stderr
    except subprocess.TimeoutExpired as e:
        code, stdout, stderr = 124, "", str(e.stderr or b"")[-800:]
    print(f"ntt_conformance {name}: wall time {time.time() - t0:.1f} s, exit code {code}")
    if code not in (0, 1):             # a signal (134, 139, -6, -11), the limit (124, 137), an exception (3), anything else
        _stopped.append(f"the child of configuration {name} ended with {code}: {stderr[-800:]}")
        pytest.fail(_stopped[0])
    lines = [json.loads(ln) for ln in stdout.splitlines() if ln.startswith("{")]
    _results[name] = {f"{'plan=' if r.get('plan_only') else ''}{r['log_n']}:{r['count']}": r for r in lines}
    return _results[name]


@pytest.mark.parametrize("name,shape", [(n, s) for n, (_, shapes) in CONFIGS.items() for s in shapes])
def test_forced_plan_whole_outputs(name, shape):
    res = run_config(name)
    assert shape in res, f"{name}: the child reported nothing for {shape}"
    tile_log, persistent = CONFIGS[name][1][shape]
    check_plan(res[shape]["plan"], int(shape.split("=")[-1].split(":")[0]), tile_log, persistent)
    if shape.startswith("plan="):
        return
    assert res[shape]["arrays"] >= 4 * len(nc.INPUTS)
    assert not res[shape]["mismatches"], "\n".join(res[shape]["mismatches"])
