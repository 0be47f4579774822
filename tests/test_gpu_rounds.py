"""The O(n) kernels of the five prover rounds (cap_amd/csrc/plonk_kernels.hpp) on the MI355X, one by one: the scans, the
permutation grand product, k_kx_columns, both forms of k_quotient, k_quotient_top, the degree check, power tables,
evaluations, the linear combination, the division by a linear factor, the copies and the blinders.  Whole proofs reach
them only with random witnesses, challenges nobody chose and domains up to 2^15; here tests/hip/roundcheck - built by
build() from the kernels' own header, launched through round_launch.hpp as the prover launches them - runs the cases of
tests/round_model.py: lengths on both sides of every block boundary up to 131073 (k_scan_totals' second trip), beta = 0,
challenges and tables at 0, 1, r - 1, and images whose 29-bit limbs are all saturated, inside each input's contract.
Expected values are Python integers (tests/test_round_model.py checks the models against the oracle without a GPU).
Checked per case: every element of every result, its representation (k_quotient's results below 2 r, all others
canonical), and that everything outside the results keeps the sentinel.

The binary runs ONCE, as one fresh child process under its own time limit; the tests only parse its result file.
TIME_LIMIT_S is the floor tests/test_gpu_devcheck.py uses for a binary of this kind; MEASURED_S is the binary's wall time
on the MI355X (0.56 s for the 117 cases, 111 MB of case file), below a fifth of the limit."""
import os
import subprocess
import time

import pytest

from tests import round_model as rm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "hip", "roundcheck")
MEASURED_S = 0.56
TIME_LIMIT_S = 60.0


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert os.path.exists(EXE), "tests/hip/roundcheck is missing: build() makes it (make -C cap_amd/csrc)"
    d = tmp_path_factory.mktemp("roundcheck")
    groups = {g: make() for g, make in rm.GROUPS.items()}
    cases = [c for g in rm.GROUPS for c in groups[g]]
    inp, res = str(d / "cases.bin"), str(d / "results.bin")
    rm.write_cases(inp, cases)
    t0 = time.time()
    try:
        out = subprocess.run([EXE, inp, res], capture_output=True, text=True, timeout=TIME_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"roundcheck did not finish within {TIME_LIMIT_S} s: {(e.stderr or b'')[-800:]}")
    wall = time.time() - t0
    print(f"roundcheck: {len(cases)} cases, {os.path.getsize(inp) / 1e6:.0f} MB, wall time {wall:.2f} s")
    assert out.returncode == 0, f"roundcheck ended with {out.returncode}: {out.stderr[-1200:]}"
    results = rm.read_results(res, cases)
    os.remove(inp)
    os.remove(res)
    by_id = dict(zip((id(c) for c in cases), results))
    return {"groups": {g: [(c,) + by_id[id(c)] for c in groups[g]] for g in rm.GROUPS}, "wall": wall}


@pytest.mark.parametrize("group", list(rm.GROUPS))
def test_device_results_match_the_model(run, group):
    rows = run["groups"][group]
    assert rows
    bad = [line for c, rc, dst in rows for line in rm.check_case(c, rc, dst)]
    assert not bad, f"{len(bad)} complaints, first:\n" + "\n".join(bad[:12])


def test_a_real_beta_of_zero_is_left_to_the_direct_form(run):
    """the folded launch leaves the rows of the proof with beta = 0 holding the sentinel; the direct launch with
    only_unfoldable = 1 writes those rows and no others"""
    seen = set()
    for c, rc, dst in run["groups"]["quotient"]:
        m, P, five, forms, only_unfoldable = c.params[:5]
        if forms == 3 or (forms == 2 and not only_unfoldable):
            continue
        assert rc == 0, c.name
        written = [bool((dst[p * m:(p + 1) * m] != rm.io.SENTINEL).any()) for p in range(P)]
        assert written == ([True, False, True] if forms == 1 else [False, True, False]), c.name
        seen.add((m, five, forms))
    assert seen == {(m, five, forms) for m in (96, 192) for five in (0, 1) for forms in (1, 2)}


def test_the_run_stays_below_a_fifth_of_its_limit(run):
    assert run["wall"] < TIME_LIMIT_S / 5, f"roundcheck took {run['wall']:.2f} s: split the case file"
