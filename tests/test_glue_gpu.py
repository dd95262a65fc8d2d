"""GPU: the edge-weight kernels of csrc/csr.hip (k_edge_renorm, k_transpose_vals, k_csr_invdeg) and the layout kernels of
csrc/exec.hip (k_cat_cols, k_transpose) against tests/glue_ref.py.  cgc_edge_renorm, cgc_csr_transpose_vals, cgc_cat_cols and
cgc_transpose bit for bit; cgc_csr_invdeg within (deg + 1) * 2^-24 relative to float64 (derived there), its excess printed.
tests/test_glue_ref_cpu.py asserts what the graphs and cases reach and that the mutants are rejected.

Every call goes straight to the library into canary-surrounded buffers (the slots of val and t_val beyond nnz, padding columns and
spare rows included), twice on fresh buffers -- aligned and one float past a 16-byte boundary -- with identical bits.

Measured on an MI355X, the largest excess of cgc_csr_invdeg: 0.331 with values (n = 257), 0.125 without; the float32 restatement on
the CPU gives the same figures."""
import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def twice(run):
    """run(Place) -> list of numpy arrays, on an aligned and a misaligned placement: containment both times, identical bits."""
    first, second = G.Place(DEV, 'aligned'), G.Place(DEV, 'misaligned')
    o1, o2 = run(first), run(second)
    first.check(), second.check()
    for a, b in zip(o1, o2):
        assert G.same_bits(a, b), 'the second launch differs from the first'
    return o1


@pytest.mark.parametrize('n', G.CSR_N)
def test_edge_weights(n):
    g = G.graph(n)

    def run(P):
        o = G.run_csr(hip(), P, g)
        assert o.rc == [0, 0, 0, 0]
        return [o.val, o.t_val, o.inv_w, o.inv_deg]
    val, t_val, inv_w, inv_deg = twice(run)
    want = G.edge_renorm(g)
    assert G.same_bits(val, want), 'cgc_edge_renorm'
    assert G.same_bits(t_val, G.transpose_vals(g, want)), 'cgc_csr_transpose_vals'
    ex = G.Excess()
    ex.add('invdeg/val', G.excess_invdeg(g, inv_w, G.invdeg(g, g.w)))
    ex.add('invdeg/deg', G.excess_invdeg(g, inv_deg, G.invdeg(g, None)))
    print('GLUE n=%d: %s' % (n, ex.line()))
    assert all(e <= 1.0 for e in ex.values()), ex


def test_no_rows_no_write():
    g = G.graph(255)

    def run(P):
        o = G.run_csr(hip(), P, g, n=0)
        assert o.rc == [0, 0, 0, 0]
        return [o.val, o.t_val, o.inv_w, o.inv_deg]
    for a in twice(run):
        assert (a == G.CANARY).all()


@pytest.mark.parametrize('accumulate', (0, 1))
@pytest.mark.parametrize('case', G.CAT_CASES, ids=lambda c: c.name)
def test_cat_cols(case, accumulate):
    def run(P):
        rc, dst = G.run_cat(hip(), P, case, accumulate)
        assert rc == 0
        return [dst]
    dst, = twice(run)
    assert G.same_bits(dst, G.cat_cols(case, accumulate))


@pytest.mark.parametrize('nsrc', (0, 5))
def test_cat_cols_refuses_source_counts(nsrc):
    case = G.CAT_CASES[4]

    def run(P):
        rc, dst = G.run_cat(hip(), P, case, 0, nsrc=nsrc)
        assert rc != 0
        return [dst]
    dst, = twice(run)
    assert (dst == G.CANARY).all()


@pytest.mark.parametrize('rows,cols', G.TRANSPOSE_CASES)
def test_transpose(rows, cols):
    def run(P):
        rc, dst = G.run_transpose(hip(), P, rows, cols)
        assert rc == 0
        return [dst]
    dst, = twice(run)
    assert G.same_bits(dst, G.transpose_input(rows, cols).T)
