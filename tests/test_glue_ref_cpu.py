"""CPU: the references of tests/glue_ref.py -- that the restated launches are the ones in csrc/csr.hip and csrc/exec.hip, that the
graphs and layout cases reach every route (a partly filled last workgroup, a second workgroup, the grid-stride second pass, cut and
whole transpose tiles), that the float32 twin of cgc_csr_invdeg stays within the derived allowance, and that every mutant is rejected
on every case where it can show."""
import numpy as np
import pytest

import glue_ref as G


def test_constants_are_the_sources():
    k = G.source_constants()
    assert (k.row_block, k.cat_block, k.cat_cap, k.tile, k.max_src) == (256, 256, 4096, 32, 4)
    assert [G.route_rows(n) for n in (0, 1, 255, 256, 257)] == [(0, 0), (1, 1), (1, 255), (1, 256), (2, 1)]
    assert [G.route_cat(c.rows, sum(c.widths))[1] for c in G.CAT_CASES] == [1] * 6 + [2]
    assert G.route_cat(1100, 1000) == (4096, 2) and 1100 * 1000 > 4096 * 256
    assert [G.route_transpose(*rc) for rc in G.TRANSPOSE_CASES] == [(1, 1, True), (2, 1, True), (1, 1, False), (3, 2, True), (1, 3, True)]


@pytest.mark.parametrize('n', G.CSR_N)
def test_graphs_hold_what_they_promise(n):
    g = G.graph(n)
    assert g.rowptr[0] == 0 and g.rowptr[-1] == g.nnz and g.cap == g.nnz + G.SPARE and np.isnan(g.w[g.nnz:]).all()
    assert (g.col[:g.nnz] >= 0).all() and (g.col[:g.nnz] < n).all()
    if n == 1:
        assert g.kind == ['self_only'] and g.nnz == 1
        return
    seen = {(kind, int(d)) for kind, d in zip(g.kind, g.deg)}
    assert {kind for kind, _ in seen} == set(G.KINDS)
    for kind in ('no_self', 'below_one', 'exactly_one'):        # every degree of the table, 0 turning the row into an empty one
        assert {d for kd, d in seen if kd == kind} == set(G.DEGREES) - {0}, kind
    sums = G.invdeg(g, g.w)
    for r in range(n):
        cols = g.col[g.rowptr[r]:g.rowptr[r + 1]]
        w = g.w[g.rowptr[r]:g.rowptr[r + 1]].astype(np.float64)
        assert len(set(cols.tolist())) == len(cols)
        assert (r in cols) == (g.kind[r] in ('self_only', 'below_one', 'exactly_one'))
        if g.kind[r] == 'exactly_one':
            assert w.sum() == 1.0 and sums[r] == 1.0
        if g.kind[r] == 'below_one':
            assert abs(w.sum() - 0.6) < 1e-6 and sums[r] == 1.0
    # the transposed slot order is a permutation that sorts the columns, row order kept inside a column
    perm = g.t_perm[:g.nnz]
    assert sorted(perm.tolist()) == list(range(g.nnz)) and (np.diff(g.col[perm]) >= 0).all()
    assert np.array_equal(np.bincount(g.col[:g.nnz], minlength=n), np.diff(g.t_rowptr))


@pytest.mark.parametrize('n', G.CSR_N)
def test_csr_references_and_twin(n):
    g = G.graph(n)
    val = G.edge_renorm(g)
    assert (val[g.nnz:] == G.CANARY).all()
    for r in range(n):                                  # against the float64 formula of _re_norm_adj: p on the diagonal, (1 - p) / off
        s, e = g.rowptr[r], g.rowptr[r + 1]
        off = np.count_nonzero(g.col[s:e] != r)
        want = np.where(g.col[s:e] == r, 0.4, 0.6 / max(off, 1))
        assert np.allclose(val[s:e], want, rtol=3 * G.U, atol=0)
    t = G.transpose_vals(g, val)
    assert (t[g.nnz:] == G.CANARY).all() and np.array_equal(np.sort(t[:g.nnz]), np.sort(val[:g.nnz]))
    for w in (g.w, None):
        want = G.invdeg(g, w)
        twin = G.invdeg(g, w, dtype=np.float32)
        e = G.excess_invdeg(g, twin, want)
        print('GLUE invdeg twin n=%d %s: excess %.3f' % (n, 'val' if w is not None else 'deg', e))
        assert e <= 1.0
        if w is None:
            assert G.same_bits(twin, want.astype(np.float32))


@pytest.mark.parametrize('mutant', G.CSR_MUTANTS)
def test_csr_mutants_are_rejected(mutant):
    for n in G.CSR_N:
        g = G.graph(n)
        val = G.edge_renorm(g)
        if mutant.startswith('renorm'):
            bad = not G.same_bits(G.edge_renorm(g, mutant=mutant), val)
            assert bad == (n > 1), n                    # shows in every row with a self-loop and a neighbour
        elif mutant == 'tvals_identity':
            assert G.same_bits(G.transpose_vals(g, val, mutant=mutant), G.transpose_vals(g, val)) == (n == 1)
        else:
            got = G.invdeg(g, g.w, dtype=np.float32, mutant=mutant)
            shows = n > 1 or mutant == 'invdeg_no_clamp'         # n = 1: one weight below 1
            assert (G.excess_invdeg(g, got, G.invdeg(g, g.w)) > 1.0) == shows, n


def test_layout_references():
    for case in G.CAT_CASES:
        c = G.cat_inputs(case)
        plain, acc = G.cat_cols(case, 0), G.cat_cols(case, 1)
        at = 0
        for a, w in zip(c.srcs, case.widths):
            assert np.array_equal(plain[:, at:at + w], a)
            at += w
        assert at == plain.shape[1] and np.array_equal(acc, c.dst0 + plain)
    assert {len(c.widths) for c in G.CAT_CASES} == {1, 2, 3, 4} and any(1 in c.widths for c in G.CAT_CASES)
    assert any(0 in c.widths[1:-1] for c in G.CAT_CASES)


@pytest.mark.parametrize('mutant', G.CAT_MUTANTS)
def test_layout_mutants_are_rejected(mutant):
    shown = 0
    for case in G.CAT_CASES:
        for accumulate in (0, 1):
            can = {'cat_zero_width_shift': 0 in case.widths[:-1] and case.widths[case.widths.index(0) + 1] > 1,
                   'cat_accumulate_ignored': bool(accumulate),
                   'cat_second_pass_dropped': G.route_cat(case.rows, sum(case.widths))[1] > 1}[mutant]
            differs = not G.same_bits(G.cat_cols(case, accumulate, mutant=mutant), G.cat_cols(case, accumulate))
            assert differs == can, (case.name, accumulate)
            shown += can
    assert shown
