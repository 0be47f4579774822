"""The DEFERRED form of the witness solver's schedule (capgpu_plonk_key_set_solve_form, include/capgpu.h) in Python: which
variables are carried as pairs, where the flush levels go, and every field of capgpu_solve_form_info - the definition the
library's figures are compared with in tests/test_gpu_solve_defer.py.  The VALUES need no model of their own: either form
gives walk_io / walk_hints of the existing models.  A helper module: it holds no test.

The direct schedule is restated here from the rule (levels and kinds only, for circuits and lists the rule accepts), not
taken from the library."""
import heapq

from cap_amd import bench_utils as bu
from cap_amd.lib import HINT_BITS, HINT_INV0

R = bu.R
Q_LC, Q_MUL, Q_HASH, Q_O, Q_C, Q_ECC = 0, 4, 6, 10, 11, 12
OUT_MUL, OUT_INV, ROOT5, INV0, ISZERO, BITS, LIN = range(7)
GROUP = 32                                     # pairs per flush item
_RANK = {OUT_MUL: 0, LIN: 1, OUT_INV: 2, ROOT5: 3, INV0: 4, ISZERO: 5, BITS: 6}


def direct_levels(sc, given_ids, hints, flags):
    """-> the direct schedule: a list of levels, each a list of items (kind, row or hint index, wire or chunk) in the
    schedule's order"""
    n, sel, wv, nv = sc.n, sc.selectors, sc.wire_vars, sc.num_vars
    level = [None] * nv
    for v in given_ids:
        level[v] = 0
    by_src = {}
    for h, (_, src, _) in enumerate(hints):
        by_src.setdefault(src, []).append(h)
    ready, items = [], []

    def valued(v):
        for h in by_src.get(v, ()):
            heapq.heappush(ready, h)

    def fire():
        while ready:
            h = heapq.heappop(ready)
            kind, src, tg = hints[h]
            for t in tg:
                level[t] = level[src] + 1
            k = BITS if kind == HINT_BITS else INV0 if kind == HINT_INV0 else ISZERO
            items.extend((level[src] + 1, k, h, g) for g in range((len(tg) + 31) // 32))
            for t in tg:
                valued(t)

    for v in given_ids:
        valued(v)
    fire()
    for j in range(n):
        ids = [wv[i][j] for i in range(5)]
        unknown = [v for v in dict.fromkeys(ids) if level[v] is None]
        if not unknown or (j < sc.num_inputs and flags & 2):
            continue
        assert len(unknown) == 1 and j >= sc.num_inputs, j
        u = unknown[0]
        where = [i for i in range(5) if ids[i] == u]
        q = lambda s: sel[s][j] % R                              # noqa: E731
        if where == [4] and (q(Q_O) or q(Q_ECC)):
            kind = OUT_INV if q(Q_ECC) else OUT_MUL
        elif len(where) == 1 and q(Q_HASH + where[0]) and not q(Q_LC + where[0]) and not q(Q_MUL + where[0] // 2) and not q(Q_ECC):
            kind = ROOT5
        else:
            assert flags & 1 and len(where) == 1 and q(Q_LC + where[0]), j
            kind = LIN
        level[u] = 1 + max(level[v] for v in ids if v != u)
        items.append((level[u], kind, j, where[0]))
        valued(u)
        fire()
    items.sort(key=lambda it: (it[0], _RANK[it[1]], it[2], it[3]))
    levels = [[] for _ in range(max((it[0] for it in items), default=0))]
    for lvl, kind, idx, w in items:
        levels[lvl - 1].append((kind, idx, w))
    return levels


def defer_model(sc, given_ids, hints, flags):
    """-> dict(deferred=[variables in the order they are deferred], flush_before=[direct level indices (0-based) a flush level
    stands in front of; len(levels) for the final one], flush_sizes=[variables each flush resolves], masks={row: mask of
    pending cells}, slots=largest PENDING, info_deferred=..., info_direct=... (capgpu_solve_form_info as dicts))"""
    n, sel, wv = sc.n, sc.selectors, sc.wire_vars
    levels = direct_levels(sc, given_ids, hints, flags)
    pending, pend = [], set()
    deferred, flush_before, flush_sizes, masks = [], [], [], {}
    out_levels = 0
    inv_direct = inv0_levels = flush_items = slots = 0

    def flush(at):
        nonlocal flush_items, out_levels
        flush_before.append(at)
        flush_sizes.append(len(pending))
        flush_items += (len(pending) + GROUP - 1) // GROUP
        out_levels += 1
        pending.clear()
        pend.clear()

    for l, items in enumerate(levels):
        need = False
        for kind, idx, w in items:
            if kind in (INV0, ISZERO, BITS):
                need |= hints[idx][1] in pend
            elif kind in (ROOT5, LIN):
                need |= any(wv[i][idx] in pend for i in range(5))
            else:
                need |= any(wv[i][idx] in pend and sel[Q_HASH + i][idx] % R for i in range(4))
        inv_direct += any(k in (OUT_INV, INV0) for k, _, _ in items)
        inv0_levels += any(k == INV0 for k, _, _ in items)
        if need and pending:
            flush(l)
        new = []
        for kind, idx, w in items:                               # (OUT_MUL rows stand before OUT_INV rows in a level)
            if kind in (OUT_MUL, OUT_INV):
                mask = sum(1 << i for i in range(4) if wv[i][idx] in pend)
                if kind == OUT_INV or mask:
                    masks[idx] = mask
                    new.append(wv[4][idx])
        deferred += new
        pending += new
        pend.update(new)
        slots = max(slots, len(pending))
        out_levels += 1
    if pending:
        flush(len(levels))
    common = dict(inv_levels_direct=inv_direct, inv_levels_deferred=len(flush_before) + inv0_levels)
    info_deferred = dict(form=1, deferred_vars=len(deferred), frac_rows=len(deferred), flush_levels=len(flush_before),
                         flush_items=flush_items, levels=out_levels, **common)
    info_direct = dict(form=0, deferred_vars=0, frac_rows=0, flush_levels=0, flush_items=0, levels=len(levels), **common)
    return dict(deferred=deferred, flush_before=flush_before, flush_sizes=flush_sizes, masks=masks, slots=slots,
                info_deferred=info_deferred, info_direct=info_direct)
