"""CPU: the float64 reference of tests/spmm_ref.py against a dense product built independently and against the float32 restatement
(oracle/flat_ref.TorchKernels.spmm); the bookkeeping that the case list of tests/test_spmm_fp64_gpu.py reaches every kernel instance,
every branch of the block-id arithmetic, every tail count and every staging round; the sensitivity of the yardstick -- each kind of
subtly wrong result is reported as an excess above 1 on every case that has the operand; the float32 restatement within the derived
allowance on every case (the bound is attainable by a correct float32 implementation: its largest excess over the list is
0.47); and the constants spmm_ref.route() assumes, parsed from csrc/spmm.hip and csrc/common.hpp."""
import os
import re

import numpy as np
import pytest
import torch

import spmm_ref as S
from oracle.flat_ref import TorchKernels

TWIN = TorchKernels()
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cgc-net_amd', 'csrc')


# ---------------------------------------------------------------------------------------------- reference against independent forms
@pytest.mark.parametrize('combo', S.ALL_COMBOS, ids=S.combo_name)
def test_reference_is_the_dense_product(combo):
    """post * ((W o pre) @ x) with W assembled entry by entry (duplicate edges add up), and the float32 restatement to float32 accuracy."""
    c = S.case(13, combo, 'B5')
    i, g = S.inputs(c), S.graph_of(c)
    x = torch.nan_to_num(i.x[:, :c.width], nan=0.0)
    ref = S.spmm(g.rowptr, g.col, i.perm, i.val, i.pre, i.post, x, g.n)
    W, Wa = np.zeros((g.n, g.n)), np.zeros((g.n, g.n))
    rp, col = g.rowptr.numpy(), g.col.numpy()
    for r in range(g.n):
        for k in range(rp[r], rp[r + 1]):
            w = 1.0
            if i.val is not None:
                w = float(i.val[int(i.perm[k])] if i.perm is not None else i.val[k])
            if i.pre is not None:
                w *= float(i.pre[col[k]])
            W[r, col[k]] += w
            Wa[r, col[k]] += abs(w)
    post = np.ones(g.n) if i.post is None else i.post.double().numpy()
    dense = post[:, None] * (W @ x.double().numpy())
    bound = np.abs(post)[:, None] * (Wa @ np.abs(x.double().numpy()))
    assert float(np.abs(ref.want.numpy() - dense).max()) <= 1e-12 * max(1.0, float(np.abs(dense).max()))
    assert float(np.abs(ref.terms.numpy() - bound).max()) <= 1e-12 * float(bound.max())
    assert bool((ref.terms >= ref.want.abs() * (1 - 1e-12)).all())
    assert np.array_equal(ref.deg.numpy(), g.deg.astype(np.float64))
    got = torch.zeros(g.n, c.width)
    TWIN.spmm(g.rowptr, g.col, i.perm, i.val, i.pre, i.post, x, got, g.n, c.width)
    assert float((got.double() - ref.want).abs().max()) <= 1e-5 * float(ref.want.abs().max())


def test_graph_builder_keeps_its_promises():
    for c in S.CASES:
        g, i = S.graph_of(c), S.inputs(c)
        rp, col = g.rowptr.numpy().astype(np.int64), g.col.numpy()
        gp = g.gptr.numpy()
        assert np.array_equal(rp[1:] - rp[:-1], [c.degrees[(r + c.phase) % len(c.degrees)] for r in range(g.n)])
        owner = np.repeat(np.arange(g.B), g.counts)
        rows = np.repeat(np.arange(g.n), g.deg)
        assert np.array_equal(owner[col], owner[rows]), 'a column outside the row\'s own graph'
        assert len(g.unref) == sum(1 for s in g.counts if s >= 2) and not set(g.unref) & set(col.tolist())
        assert all(gp[owner[u]] <= u < gp[owner[u] + 1] for u in g.unref)
        assert len(np.unique(col)) < len(col), 'no duplicate edge'
        assert len(g.val) > len(col) and len(set(g.perm.tolist())) == len(col) and int(g.perm.max()) < len(g.val)
        for t in (g.val, g.pre, g.post):
            a = t.abs()
            assert float(a.min()) >= 0.3 and float((a - 1).abs().min()) >= 0.2 and bool((t < 0).any()) and bool((t > 0).any())
        assert bool(torch.isnan(i.x[g.unref]).all()) and bool(torch.isnan(i.x[:, c.width:]).all())
        finite = np.setdiff1d(np.arange(g.n), g.unref)
        assert bool(torch.isfinite(i.x[finite, :c.width]).all())
        assert bool(torch.isfinite(S.reference_of(c).want).all())


# ---------------------------------------------------------------------------------------------- bookkeeping over the case list
def test_case_list_visits_every_instance():
    """BOOKKEEPING: spmm_ref.route() restates launch_gather and has to follow it when it changes.  It is used here only: to assert
    that the case list reaches every kernel instance and every branch that the block-id arithmetic, the tails and the staging loop have."""
    seen = set()
    for c in S.CASES:
        g = S.graph_of(c)
        degs = set(int(d) for d in g.deg)
        for L in S.launches(c):
            r = S.case_route(c, L.entry)
            tiles = 'several tiles' if r.n_ctiles > 1 else 'one tile'
            if r.kernel == 'k_spmm_wide':
                seen.add(('wide', r.instance, L.entry))
                seen.add(('wide', tiles))
                seen |= {('tail', min(d // S.GATHER_U, 2), d % S.GATHER_U) for d in degs}
                if r.graph_chunks:
                    seen.add(('order', L.visit, r.order_branch, 'gorder' if L.gorder else 'hint'))
            else:
                seen.add((r.kernel, r.lpr, tiles))
                seen.add((r.kernel, tiles, 'graph chunks' if r.graph_chunks else 'row chunks'))
                seen |= {(r.kernel, r.lpr, 'rounds', min(S._cdiv(d, r.lpr), 3)) for d in degs}
            if r.multi_chunk_tiles:
                seen.add((r.kernel, 'chunk > 0 with several tiles'))
                assert g.n > S.SPMM_CHUNK
            if r.graph_chunks:
                rpb = r.rows_per_block
                if any(s and s % rpb == 0 for s in g.counts) and any(s > rpb and s % rpb == 1 for s in g.counts):
                    seen.add((r.kernel, 'graph of k and of k + 1 blocks'))
                if 0 in g.counts and 1 in g.counts and g.counts[0] != g.nmax:
                    seen.add((r.kernel, 'empty graph, one-node graph, largest not first'))
    want = {('k_spmm<4>', lpr, 'one tile') for lpr in (8, 16, 32)}
    want |= {('k_spmm<1>', lpr, 'one tile') for lpr in (8, 16, 32, 64)} | {('k_spmm<1>', 64, 'several tiles')}
    want |= {('k_spmm<1>', 'several tiles', 'graph chunks'), ('k_spmm<1>', 'several tiles', 'row chunks')}
    want |= {('wide', inst, entry) for inst in ((False, False, False), (False, False, True), (True, False, False), (True, False, True),
                                                 (True, True, False), (True, True, True)) for entry in ('flat', 'graphs')}
    want |= {('wide', 'one tile'), ('wide', 'several tiles')}
    want |= {('order', v, br, 'hint') for v in (0, 1, 2) for br in ('formula', 'reversal')}
    want |= {('order', 0, br, 'gorder') for br in ('formula', 'reversal')}
    want |= {(k, 'chunk > 0 with several tiles') for k in ('k_spmm<1>', 'k_spmm_wide')}
    want |= {('tail', full, cnt) for full in (0, 1, 2) for cnt in range(S.GATHER_U)}
    want |= {('k_spmm<4>', lpr, 'rounds', r) for lpr in (8, 16, 32) for r in (1, 2, 3)}
    want |= {('k_spmm<1>', lpr, 'rounds', r) for lpr in (8, 16, 32, 64) for r in (1, 2, 3)}
    want |= {(k, what) for k in ('k_spmm<1>', 'k_spmm_wide')
             for what in ('graph of k and of k + 1 blocks', 'empty graph, one-node graph, largest not first')}
    assert not want - seen, 'not reached by any case: %r' % sorted(want - seen, key=repr)
    # the width of a case decides its kernel; a misaligned operand or a row stride that is no multiple of 4 sends it to the scalar one
    for c in S.CASES:
        for L in S.launches(c):
            r = S.case_route(c, L.entry)
            forced = bool(c.mis) or c.ld % 4 != 0
            expect = ('k_spmm<1>' if forced or c.width in S.SCALAR_WIDTHS else 'k_spmm_wide' if c.width >= 132 else 'k_spmm<4>')
            assert r.kernel == expect, (c.name, r.kernel)
    assert {c.width for c in S.CASES if c.mis} == {4, 64, 260}
    assert all(S.case_route(c, 'graphs').graph_chunks for c in S.CASES if c.ld == c.width + 1)
    assert S.route(128, 128, True, True, True, False, False, 600, 8, 300).kernel == 'k_spmm<4>'
    assert S.route(132, 132, True, True, True, False, False, 600, 8, 300).kernel == 'k_spmm_wide'
    assert S.route(256, 256, True, True, True, False, False, 600, 8, 300).graph_chunks is False
    assert S.route(260, 260, True, True, True, False, False, 600, 8, 300).graph_chunks is True
    assert S.route(64, 64, False, True, True, False, False, 600, 8, 300).n_ctiles == 1
    assert S.route(65, 65, True, True, True, False, False, 600, 8, 300).n_ctiles == 2
    # both entry points and every degree of the list on each of the three kernels
    for kernel in ('k_spmm<4>', 'k_spmm<1>', 'k_spmm_wide'):
        for entry in ('flat', 'graphs'):
            degs = set()
            for c in S.CASES:
                if any(L.entry == entry for L in S.launches(c)) and S.case_route(c, entry).kernel == kernel:
                    degs |= set(int(d) for d in S.graph_of(c).deg)
            assert degs >= set(S.DEGREES), (kernel, entry)
    assert set(S.DEGREES) >= {0, 1, 2, 7, 8, 9, 10, 15, 16, 17, 18, 19, 26, 27, 28, 31, 32, 33, 63, 64, 65, 130}


def test_route_assumes_the_constants_of_the_source():
    """A retune of a launch constant fails here instead of silently shrinking what the case list covers."""
    with open(os.path.join(CSRC, 'spmm.hip')) as f:
        hip = f.read()
    with open(os.path.join(CSRC, 'common.hpp')) as f:
        hpp = f.read()
    const = lambda name, text: [int(v) for v in re.findall(r'\b%s\s*=\s*(\d+)\s*[,;]' % name, text)]
    assert const('GATHER_U', hip) == [S.GATHER_U]
    assert const('SPMM_PASSES', hip) == [S.SPMM_PASSES]
    assert const('SPMM_CHUNK', hip) == [S.SPMM_CHUNK]
    assert const('SPMM_RUN', hip) == [S.SPMM_RUN]
    assert re.findall(r'#define\s+CGC_BLOCK\s+(\d+)', hpp) == [str(64 * S.WAVES)]
    lpr = re.search(r'static inline int pick_lpr\(int chunks\)\s*\{\s*return (.*?);\s*\}', hpp).group(1)
    assert ' '.join(lpr.split()) == 'chunks <= 8 ? 8 : chunks <= 16 ? 16 : chunks <= 32 ? 32 : 64'
    assert S.LPR_STEPS == (8, 16, 32) and [S.pick_lpr(v) for v in (1, 8, 9, 16, 17, 32, 33, 285)] == [8, 8, 16, 16, 32, 32, 64, 64]
    flat = ' '.join(hip.split())
    assert 'const bool vec = (width % 4 == 0) && (ld % 4 == 0) && aligned16(x) && aligned16(out);' in flat
    assert 'const int rows_per_block = 4 * rpw * SPMM_PASSES;' in flat and 'const int rpb = 4 * SPMM_RUN;' in flat
    assert 'if (gptr != nullptr && n_ctiles > 1) {' in flat and 'if (vec && lpr == 64) {' in flat
    assert flat.count('k_spmm_wide<GATHER_U, V, P, Q>') == 1 and flat.count('WIDE_LAUNCH(') == 7      # the macro and six instances


# ---------------------------------------------------------------------------------------------- the yardstick discriminates
@pytest.mark.parametrize('c', S.CASES, ids=lambda c: c.name)
def test_yardstick_flags_every_mutation(c):
    muts = S.mutations(c)
    v, p, q, s = c.combo
    expect = {'drop the last edge of a row', 'duplicate an edge'}
    expect |= {'val[k] for val[perm[k]]'} if v and p else set()
    expect |= {'pre by row'} if q else set()
    expect |= {'post omitted'} if s else set()
    expect |= {'column tile shifted by a lane'} if c.width > S.case_route(c, 'graphs').VEC else set()
    assert set(muts) == expect
    for name, (got, ref) in muts.items():
        assert S.excess(got.float(), ref) > 1.0, '%s: not noticed on %s' % (name, c.name)
    ref = S.reference_of(c)
    assert S.excess(ref.want.float(), ref) <= 0.5          # the reference rounded to float32 passes, with room
    nan = ref.want.float().clone()
    nan[-1, -1] = float('nan')
    assert S.excess(nan, ref) == float('inf')
    if bool((ref.terms == 0).any()):
        dirty = ref.want.float().clone()
        dirty[ref.terms == 0] = 1e-30
        assert S.excess(dirty, ref) == float('inf')


# ---------------------------------------------------------------------------------------------- the float32 restatement
@pytest.mark.parametrize('c', S.CASES, ids=lambda c: c.name)
def test_float32_restatement_is_within_the_allowance(c):
    """The same call sequence as on the GPU, on the float32 torch restatement: every launch within the allowance, the padding and the
    spare rows at their canary."""
    def launch(run):
        P = S.Places('cpu', c.mis)
        o = run(P)
        P.check()
        return o
    ex, outs = S.check_case(TWIN, c, launch)
    print('SPMM twin %s: %s' % (c.name, ex.line()))
    assert ex and all(e <= 1.0 for e in ex.values()), ex
    assert all(bool(torch.isfinite(o).all()) for o in outs.values())
