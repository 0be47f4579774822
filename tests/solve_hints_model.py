"""The witness solver's rule WITH HINTS (include/capgpu.h) in Python integers - the definition the device is compared with
in tests/test_gpu_solve_hints.py.  The row rule is tests/test_gpu_solve.py's `walk`; added here: the firing step (the ready
hint of lowest index, until none is ready, before row 0 and after every defining row), the three hint values, and the item
counts.  A helper module: it holds no test."""
import heapq

from cap_amd import bench_utils as bu
from cap_amd.lib import HINT_BITS, HINT_INV0, HINT_ISZERO
from tests.test_gpu_solve import E5, Q_ECC, Q_HASH, Q_LC, Q_MUL, Q_O, rest_of

R = bu.R


def hint_values(kind, x, count):
    """the targets' values for the source value x (0 <= x < R)"""
    if kind == HINT_BITS:
        return [(x >> i) & 1 for i in range(count)]              # bits beyond count are dropped
    if kind == HINT_INV0:
        return [pow(x, R - 2, R)]                                # 0 -> 0
    return [1 if x == 0 else 0]


def walk_hints(sc, given_ids, given_vals, hints):
    """hints: (kind, src, [targets]) -> (value per variable, status (kind, row), solver info dict, hint info dict);
    raises ValueError(text) where the rule refuses"""
    n, sel, wv, nv = sc.n, sc.selectors, sc.wire_vars, sc.num_vars
    if len(set(given_ids)) != len(given_ids):
        raise ValueError("given twice")
    if any(v >= nv for v in given_ids):
        raise ValueError("num_vars is")
    val = [None] * nv
    level = [0] * nv
    def_row = {}
    for v, x in zip(given_ids, given_vals):
        val[v] = x % R
    owner, given_set = {}, set(given_ids)
    for h, (kind, src, tg) in enumerate(hints):
        if kind not in (HINT_BITS, HINT_INV0, HINT_ISZERO):
            raise ValueError(f"hint {h}: unknown kind {kind}")
        if not 1 <= len(tg) <= (254 if kind == HINT_BITS else 1):
            raise ValueError(f"hint {h}: count {len(tg)} is out of range")
        if src >= nv:
            raise ValueError(f"hint {h}: its source variable {src}")
        for i, t in enumerate(tg):
            if t >= nv:
                raise ValueError(f"hint {h}: its target {i}, variable {t}")
            if t == src:
                raise ValueError(f"hint {h}: its target {i} is its own source variable {t}")
            if t in given_set:
                raise ValueError(f"hint {h}: its target variable {t} is given")
            if t in owner:
                raise ValueError(f"hint {h}: its target variable {t} is listed twice (hint {owner[t]} has it too)")
            owner[t] = h
    by_src = {}
    for h, (_, src, _) in enumerate(hints):
        by_src.setdefault(src, []).append(h)
    ready, fired = [], [False] * len(hints)
    widths = {}
    hinfo = dict(num_hints=len(hints), num_hinted=0, bits_hints=0, inv_hints=0, iszero_hints=0, hint_items=0)

    def valued(v):
        for h in by_src.get(v, ()):
            heapq.heappush(ready, h)

    def fire():
        while ready:
            h = heapq.heappop(ready)
            kind, src, tg = hints[h]
            for t, x in zip(tg, hint_values(kind, val[src], len(tg))):
                if val[t] is not None:
                    raise ValueError(f"hint {h}: its target variable {t} already has a value when the hint fires "
                                     f"(row {def_row[t]} defines it)")
                val[t], level[t] = x, level[src] + 1
            fired[h] = True
            items = (len(tg) + 31) // 32
            widths[level[src] + 1] = widths.get(level[src] + 1, 0) + items
            hinfo["hint_items"] += items
            hinfo["num_hinted"] += len(tg)
            hinfo[("bits_hints", "inv_hints", "iszero_hints")[kind]] += 1
            for t in tg:
                valued(t)

    for v in given_ids:
        valued(v)
    fire()
    first_zero = None
    inv_rows, root_rows, defined = 0, 0, 0
    for j in range(n):
        ids = [wv[i][j] for i in range(5)]
        unknown = []
        for v in ids:
            if val[v] is None and v not in unknown:
                unknown.append(v)
        if not unknown:
            continue
        if j < sc.num_inputs:
            raise ValueError(f"row {j} is a public-input row and its variable {unknown[0]} is not given")
        if len(unknown) >= 2:
            raise ValueError(f"row {j} holds two variables without a value, {unknown[0]} and {unknown[1]}")
        u = unknown[0]
        where = [i for i in range(5) if ids[i] == u]
        w = [0 if ids[i] == u else val[ids[i]] for i in range(5)]
        q = lambda s: sel[s][j] % R                              # noqa: E731
        if where == [4] and (q(Q_O) or q(Q_ECC)):
            den = (q(Q_O) - q(Q_ECC) * w[0] * w[1] * w[2] * w[3]) % R
            if q(Q_ECC):
                inv_rows += 1
            if den == 0:
                val[u] = 0
                first_zero = j if first_zero is None else first_zero
            else:
                val[u] = rest_of(sel, j, w) * pow(den, R - 2, R) % R
        elif len(where) == 1 and where[0] < 4 and q(Q_HASH + where[0]) and not q(Q_LC + where[0]) \
                and not q(Q_MUL + where[0] // 2) and not q(Q_ECC):
            i = where[0]
            t = (q(Q_O) * w[4] - rest_of(sel, j, w)) * pow(q(Q_HASH + i), R - 2, R) % R
            val[u] = pow(t, E5, R)
            root_rows += 1
        else:
            raise ValueError(f"row {j} cannot define its variable {u}")
        level[u] = 1 + max(level[v] for v in ids if v != u)
        def_row[u] = j
        widths[level[u]] = widths.get(level[u], 0) + 1
        defined += 1
        valued(u)
        fire()
    for h, (_, src, _) in enumerate(hints):
        if not fired[h]:
            raise ValueError(f"hint {h}: its source variable {src} never gets a value")
    info = dict(num_given=len(given_ids), num_defined=defined, levels=len(widths), widest_level=max(widths.values(), default=0),
                inv_rows=inv_rows, root_rows=root_rows)
    status = (0, 0) if first_zero is None else (1, first_zero)
    return [0 if x is None else x for x in val], status, info, hinfo
