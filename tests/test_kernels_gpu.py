"""GPU: every C-ABI entry point (through HipKernels) against the torch restatement of the kernel contract
(oracle/flat_ref.py) on the same seeded inputs.  Index work must be bit-exact; fp32 work within 1e-4 relative
(sum-order differences only).  Shapes cover: ragged graphs, widths that are / are not multiples of 4 (16-byte lanes
vs scalar lanes), rows narrower and wider than a wavefront, empty rows, duplicates, isolated nodes.
The per-element check of the row kernels (csrc/rowops.hip) against float64 is tests/test_rowops_fp64_gpu.py; that of the exact
fp32 GEMM (csrc/gemm.hip: every tile shape, kernel, layout and route) and of the reduce kernels is tests/test_gemm_fp64_gpu.py."""
import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
from oracle.flat_ref import TorchKernels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REF = TorchKernels()
TOL = 1e-4


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def close(a, b, tol=TOL, what=''):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    scale = float(b.abs().max()) if b.numel() else 0.0
    assert err <= tol * scale + 1e-7, '%s: abs err %g vs scale %g' % (what, err, scale)


def g(t):
    return None if t is None else t.to(DEV)


def rnd(*shape, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def random_graph(counts, deg=6, seed=0, dup=True, empty_rows=True):
    """Ragged batch of random directed graphs as a global int64 edge list (unsorted, with duplicates)."""
    rng = np.random.RandomState(seed)
    rows, cols, off = [], [], 0
    for n in counts:
        if n > 0:
            r = rng.randint(0, n, size=n * deg)
            c = rng.randint(0, n, size=n * deg)
            if empty_rows and n > 3:
                keep = r != 1
                r, c = r[keep], c[keep]
            rows.append(r + off)
            cols.append(c + off)
        off += n
    ei = np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int64)
    if dup:
        ei = np.concatenate([ei, ei[:, :7]], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    return torch.from_numpy(ei), off


def build_both(ei, n, add_diag):
    want = REF.csr_build(ei, n, add_diag)
    got = hip().csr_build(g(ei), n, add_diag)
    torch.cuda.synchronize()
    return want, got


def test_csr_build_drops_and_counts_out_of_range_edges():
    """A foreign Batch / bad node offset: ids outside [0, n) never reach the atomics; they are dropped and reported."""
    from cgc_net_amd.graph import BatchGraph
    ei, n = random_graph([40, 33], seed=4)
    bad = torch.tensor([[3, n, -1, 5, 7], [n + 5, 2, 4, -7, 1 << 40]], dtype=torch.int64)
    dirty = torch.cat([ei[:, :50], bad, ei[:, 50:]], dim=1)
    for add_diag in (False, True):
        want, got = build_both(ei, n, add_diag)
        _, got_dirty = build_both(dirty, n, add_diag)
        nnz = int(want['rowptr'][n])
        assert int(got['bad_edges']) == 0 and int(got_dirty['bad_edges']) == 5
        assert torch.equal(got_dirty['rowptr'].cpu(), want['rowptr']) and torch.equal(got_dirty['t_rowptr'].cpu(), want['t_rowptr'])
        for k in ('col', 'rowidx', 't_col', 't_perm'):
            assert torch.equal(got_dirty[k].cpu()[:nnz], want[k][:nnz]), k
    b = type('B', (), {})()
    b.x, b.edge_index, b._node_counts = torch.zeros(n, 4, device=DEV), g(dirty), [40, 33]
    with pytest.raises(IndexError):
        BatchGraph.from_batch(b).validate()
    b.edge_index = g(ei)
    BatchGraph.from_batch(b).validate()


@pytest.mark.parametrize('counts,add_diag', [([5, 9, 12], False), ([5, 9, 12], True), ([300, 0, 257, 64], False),
                                             ([1800, 2100, 1500], True)])
def test_csr_build_bit_exact(counts, add_diag):
    ei, n = random_graph(counts, seed=len(counts))
    want, got = build_both(ei, n, add_diag)
    nnz = int(want['rowptr'][n])
    assert torch.equal(got['rowptr'].cpu(), want['rowptr'])
    assert torch.equal(got['t_rowptr'].cpu(), want['t_rowptr'])
    for k in ('col', 'rowidx', 't_col', 't_perm'):
        assert torch.equal(got[k].cpu()[:nnz], want[k][:nnz]), k


def grouped_graph(counts, deg, seed, heavy_column=False):
    """A batch as Batch.from_data_list emits it: per graph an unsorted edge list with duplicates, the lists concatenated in graph
    order.  Returns (edge_index int64 [2, E], n, gptr, eptr)."""
    rng = np.random.RandomState(seed)
    parts, off, ecount = [], 0, []
    for n in counts:
        if n > 0:
            r, c = rng.randint(0, n, size=n * deg), rng.randint(0, n, size=n * deg)
            if n > 3:
                keep = r != 1                                     # an empty row
                r, c = r[keep], c[keep]
            if heavy_column and n > 40:
                c[: min(40, len(c))] = 2                          # one column with more sources than the in-LDS sort holds
                r[: min(40, len(r))] = np.arange(min(40, len(r))) % n
            e = np.stack([r, c]) + off
            e = np.concatenate([e, e[:, :5]], axis=1)             # duplicates
            e = e[:, rng.permutation(e.shape[1])]
        else:
            e = np.zeros((2, 0), dtype=np.int64)
        parts.append(e)
        ecount.append(e.shape[1])
        off += n
    ei = torch.from_numpy(np.concatenate(parts, axis=1).astype(np.int64))
    gptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    eptr = torch.tensor(np.concatenate([[0], np.cumsum(ecount)]), dtype=torch.int32)
    return ei, off, gptr, eptr, max(ecount)


@pytest.mark.parametrize('counts,deg,heavy', [([5, 9, 12], 3, False), ([300, 0, 257, 64], 6, True), ([1800, 2100, 1500, 1, 2500], 9, True), ([4095, 3], 3, False), ([4095, 3], 6, False),
                                               ([0, 40], 20, False)])
@pytest.mark.parametrize('renorm_p', [None, 0.4])
def test_graph_build_graph_by_graph_equals_the_general_build(counts, deg, heavy, renorm_p):
    """cgc_graph_build_local (one workgroup per graph, two launches) against cgc_graph_build on the same batch: every array bit for
    bit -- a column with 40 sources, empty graphs, a one-node graph, a graph at the node limit, duplicates, with and without the
    diagonal / edge weights of _re_norm_adj.  Then the same list with three edges that leave
    their graph: dropped and counted, everything else unchanged."""
    k = hip()
    ei, n, gptr, eptr, emax = grouped_graph(counts, deg, seed=len(counts) + deg, heavy_column=heavy)
    B, nmax = len(counts), max(counts)
    before = k.graph_local
    try:
        k.graph_local = False
        want = k.graph_build(g(ei), n, renorm_p)
        k.graph_local = True
        n_local = k.graph_local_count
        got = k.graph_build(g(ei), n, renorm_p, gptr=g(gptr), eptr=g(eptr), num_graphs=B, nmax=nmax, emax=emax)
    finally:
        k.graph_local = before
    fits = 20 * (nmax + 1) + 4 * (emax + nmax) + 4096 <= 156 * 1024 and emax + nmax <= 32767       # the envelope of the two-launch build
    assert (k.graph_local_count == n_local + 1) == fits, (nmax, emax, fits)
    torch.cuda.synchronize()
    nnz = int(want['rowptr'][n])
    assert int(got['bad_edges']) == 0 and int(want['bad_edges']) == 0
    assert torch.equal(got['rowptr'], want['rowptr']) and torch.equal(got['t_rowptr'], want['t_rowptr'])
    for key in ('col', 'rowidx', 't_col', 't_perm'):
        assert torch.equal(got[key][:nnz], want[key][:nnz]), key
    assert torch.equal(got['inv_d'], want['inv_d'])
    if renorm_p is not None:
        assert torch.equal(got['val'][:nnz], want['val'][:nnz]) and torch.equal(got['t_val'][:nnz], want['t_val'][:nnz])
    # the oracle too (the general build is itself checked against it above)
    ref = REF.csr_build(ei, n, renorm_p is not None)
    assert torch.equal(got['rowptr'].cpu(), ref['rowptr']) and torch.equal(got['col'].cpu()[:nnz], ref['col'][:nnz])
    real = [i for i, c in enumerate(counts) if c > 0]
    if fits and len(real) >= 2 and eptr[real[0] + 1] - eptr[real[0]] > 3:       # (the general build keeps an edge between two graphs of the batch)
        e0 = int(eptr[real[0]])
        dirty = ei.clone()
        other = int(gptr[real[1]])                                    # a node of ANOTHER graph, an id past the batch, a negative id
        dirty[1, e0] = other
        dirty[0, e0 + 1] = n + 3
        dirty[1, e0 + 2] = -2
        clean = torch.cat([ei[:, :e0], ei[:, e0 + 3:]], dim=1)
        ref2 = REF.csr_build(clean, n, renorm_p is not None)
        got2 = k.graph_build(g(dirty), n, renorm_p, gptr=g(gptr), eptr=g(eptr), num_graphs=B, nmax=nmax, emax=emax)
        torch.cuda.synchronize()
        nnz2 = int(ref2['rowptr'][n])
        assert int(got2['bad_edges']) == 3
        assert torch.equal(got2['rowptr'].cpu(), ref2['rowptr']) and torch.equal(got2['t_rowptr'].cpu(), ref2['t_rowptr'])
        for key in ('col', 'rowidx', 't_col', 't_perm'):
            assert torch.equal(got2[key].cpu()[:nnz2], ref2[key][:nnz2]), key


def test_graph_build_local_with_understated_sizes_builds_that_graph_empty():
    """A C-ABI caller whose nmax / emax understate one graph (the kernels size their LDS areas and per-thread arrays from them): that
    graph comes out EMPTY with all its edges counted as bad ones -- never an access past the areas -- and the other graphs as always."""
    k = hip()
    counts = [60, 400, 90]
    ei, n, gptr, eptr, emax = grouped_graph(counts, 5, seed=9)
    ec = [int(eptr[i + 1] - eptr[i]) for i in range(3)]
    for nmax_arg, emax_arg in ((100, emax), (400, ec[1] // 2)):         # too few nodes; too few edges (beyond the rounding of the areas)
        n_local = k.graph_local_count
        got = k.graph_build(g(ei), n, 0.4, gptr=g(gptr), eptr=g(eptr), num_graphs=3, nmax=nmax_arg, emax=emax_arg)
        torch.cuda.synchronize()
        assert k.graph_local_count == n_local + 1
        assert int(got['bad_edges']) == ec[1]
        keep = torch.cat([ei[:, :int(eptr[1])], ei[:, int(eptr[2]):]], dim=1)
        ref = REF.csr_build(keep, n, False)                              # (no diagonal for the refused graph's rows either)
        rp = got['rowptr'].cpu()
        g0, g1 = int(gptr[1]), int(gptr[2])
        assert bool((rp[g0:g1 + 1] == rp[g0]).all())                     # its rows are empty
        other = [r for r in range(n) if r < g0 or r >= g1]
        deg_ref = (ref['rowptr'][1:] - ref['rowptr'][:-1])
        deg_got = (rp[1:] - rp[:-1])
        has_self = torch.zeros(n, dtype=torch.bool)
        for r in other:
            s0, s1 = int(ref['rowptr'][r]), int(ref['rowptr'][r + 1])
            has_self[r] = bool((ref['col'][s0:s1] == r).any())
        for r in other:                                                  # the weighted build adds the diagonal where it was missing
            assert int(deg_got[r]) == int(deg_ref[r]) + (0 if has_self[r] else 1), r
        assert bool(torch.isfinite(got['inv_d']).all())


def test_graph_build_takes_the_general_route_outside_the_local_envelope():
    """A graph beyond cgc_graph_local_max_nodes(), and a Batch whose edge_index was replaced after the collate (the note about the
    grouping no longer describes it): the general build runs, results as always."""
    from cgc_net_amd.data import Batch, SyntheticCellGraphs
    from cgc_net_amd.graph import BatchGraph
    k = hip()
    limit = int(k.lib.cgc_graph_local_max_nodes())
    ei, n, gptr, eptr, emax = grouped_graph([limit + 1, 30], 4, seed=1)
    got = k.graph_build(g(ei), n, None, gptr=g(gptr), eptr=g(eptr), num_graphs=2, nmax=limit + 1, emax=emax)
    ref = REF.csr_build(ei, n, False)
    torch.cuda.synchronize()
    nnz = int(ref['rowptr'][n])
    assert torch.equal(got['rowptr'].cpu(), ref['rowptr']) and torch.equal(got['col'].cpu()[:nnz], ref['col'][:nnz])
    ds = SyntheticCellGraphs(3, 120, 4, base_seed=5)
    b = Batch.from_data_list([ds[i] for i in range(3)]).to(DEV)
    assert b._eptr.device.type == 'cuda' and b._etotal == b.edge_index.shape[1]
    g1 = BatchGraph.from_batch(b, 0.4)
    b2 = Batch.from_data_list([ds[i] for i in range(3)]).to(DEV)
    b2.edge_index = b2.edge_index[:, torch.randperm(b2.edge_index.shape[1], device=DEV)][:, :-4]      # regrouped and shortened behind the collate's back
    g2 = BatchGraph.from_batch(b2, 0.4)
    ref2 = REF.csr_build(b2.edge_index.cpu(), b2.x.shape[0], True)
    torch.cuda.synchronize()
    assert torch.equal(g2.rowptr.cpu(), ref2['rowptr'])
    ref1 = REF.csr_build(b.edge_index.cpu(), b.x.shape[0], True)
    assert torch.equal(g1.rowptr.cpu(), ref1['rowptr']) and int(g1.bad_edges) == 0


def test_csr_presorted_knn_input():
    from cgc_net_amd.data import Batch, SyntheticCellGraphs
    ds = SyntheticCellGraphs(3, 200, 4, base_seed=2)
    b = Batch.from_data_list([ds[i] for i in range(3)])
    n = b.x.shape[0]
    want, got = build_both(b.edge_index, n, False)
    nnz = int(want['rowptr'][n])
    assert nnz == b.edge_index.shape[1]           # k-NN output has no duplicates
    key = torch.sort(b.edge_index[0] * n + b.edge_index[1])[0]          # k-NN rows are ascending, columns by distance
    assert torch.equal(got['col'].cpu()[:nnz].long(), key % n) and torch.equal(got['rowidx'].cpu()[:nnz].long(), key // n)
    assert torch.equal(got['rowptr'].cpu(), want['rowptr'])


def _graph(counts, add_diag, seed=0):
    ei, n = random_graph(counts, seed=seed)
    s = REF.csr_build(ei, n, add_diag)
    return s, {k: (g(v) if torch.is_tensor(v) else v) for k, v in s.items()}, n


def test_edge_renorm_and_invdeg():
    s, sg, n = _graph([40, 33, 64], True)
    cap = s['cap']
    want, got = torch.zeros(cap), torch.zeros(cap, device=DEV)
    REF.edge_renorm(s['rowptr'], s['col'], n, 0.4, want)
    hip().edge_renorm(sg['rowptr'], sg['col'], n, 0.4, got)
    nnz = int(s['rowptr'][n])
    assert torch.equal(got.cpu()[:nnz], want[:nnz])      # same fp32 expression -> bit-exact
    for val_w, val_g in ((None, None), (want, got)):
        a, b = torch.zeros(n), torch.zeros(n, device=DEV)
        REF.csr_invdeg(s['rowptr'], val_w, n, a)
        hip().csr_invdeg(sg['rowptr'], val_g, n, b)
        close(b, a, 1e-6, 'invdeg')


@pytest.mark.parametrize('width', [4, 16, 18, 20, 60, 64, 180, 250, 1140])
@pytest.mark.parametrize('weighted', [False, True])
def test_spmm_forward_and_transpose(width, weighted):
    s, sg, n = _graph([130, 97, 260, 3], True, seed=width)
    cap = s['cap']
    val = vg = None
    if weighted:
        val = torch.zeros(cap)
        REF.edge_renorm(s['rowptr'], s['col'], n, 0.4, val)
        vg = g(val)
    invd = torch.zeros(n)
    REF.csr_invdeg(s['rowptr'], val, n, invd)
    x = rnd(n, width, seed=1)
    # forward aggregation with the mean divisor as post-scale
    want, got = torch.zeros(n, width), torch.zeros(n, width, device=DEV)
    REF.spmm(s['rowptr'], s['col'], None, val, None, invd, x, want, n, width)
    hip().spmm(sg['rowptr'], sg['col'], None, vg, None, g(invd), g(x), got, n, width)
    close(got, want, what='spmm fwd')
    # transpose aggregation (backward): weights through t_perm, divisor as pre-scale
    want2, got2 = torch.zeros(n, width), torch.zeros(n, width, device=DEV)
    REF.spmm(s['t_rowptr'], s['t_col'], s['t_perm'] if weighted else None, val, invd, None, x, want2, n, width)
    hip().spmm(sg['t_rowptr'], sg['t_col'], sg['t_perm'] if weighted else None, vg, g(invd), None, g(x), got2, n, width)
    close(got2, want2, what='spmm transpose')
    # graph-aware entry point (block-diagonal batch): the same results through the LDS slab kernel for wide rows
    counts = [130, 97, 260, 3]
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    got3 = torch.zeros(n, width, device=DEV)
    hip().spmm(sg['rowptr'], sg['col'], None, vg, None, g(invd), g(x), got3, n, width, g(gptr), len(counts), max(counts))
    close(got3, want, what='spmm graphs fwd')
    got4 = torch.zeros(n, width, device=DEV)
    hip().spmm(sg['t_rowptr'], sg['t_col'], sg['t_perm'] if weighted else None, vg, g(invd), None, g(x), got4, n, width,
               g(gptr), len(counts), max(counts))
    close(got4, want2, what='spmm graphs transpose')


@pytest.mark.parametrize('visit', [0, 1, 2])
def test_wide_spmm_visiting_sequences(visit):
    """Order hints and a caller-supplied visiting sequence (cgc_spmm_graphs: gorder) are scheduling only: the same bits."""
    from cgc_net_amd.graph import BatchGraph
    rng = np.random.RandomState(visit)
    counts = [int(c) for c in rng.randint(20, 140, size=16)]
    s, sg, n = _graph(counts, True, seed=7)
    gptr = g(torch.tensor(np.cumsum([0] + counts), dtype=torch.int32))
    x, W = rnd(n, 320, seed=1), 300
    xg = g(x)[:, :W]
    want = torch.zeros(n, W)
    REF.spmm(s['rowptr'], s['col'], None, None, None, None, x[:, :W].contiguous(), want, n, W)
    outs = []
    for gorder in (None, torch.tensor(rng.permutation(16), dtype=torch.int32, device=DEV)):
        out = torch.zeros(n, 320, device=DEV)[:, :W]
        hip().spmm(sg['rowptr'], sg['col'], None, None, None, None, xg, out, n, W, gptr, 16, max(counts), visit, 320, gorder)
        close(out, want, what='wide spmm visit %d' % visit)
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    big = BatchGraph(sum([5000, 4100, 6000, 4500, 4800, 5200, 4000, 5900]), [5000, 4100, 6000, 4500, 4800, 5200, 4000, 5900], DEV)
    assert sorted(big.gorder.tolist()) == list(range(8)) and BatchGraph(n, counts, DEV).gorder is None


@pytest.mark.parametrize('ordered', [True, False], ids=['grid-cell order', 'draw order'])
@pytest.mark.parametrize('width,ld,weighted', [(1140, 1152, True), (1140, 1152, False), (300, 320, True), (512, 512, False)])
def test_wide_spmm_on_cell_graphs_in_both_node_orders(width, ld, weighted, ordered):
    """The gather kernel of cgc_spmm_graphs on wide rows (A S of _diff_pool, model/network.py:207, and its transpose in the
    backward) over real cell graphs (k-NN within 100 px), their nodes in grid-cell order (with the order hint, visit bit 2) and in
    DRAW order: the forward graph and its transpose, with and without edge weights / the post scale, must equal the reference
    aggregation, and the padding columns stay untouched."""
    from cgc_net_amd.data import Batch, SyntheticCellGraphs
    from cgc_net_amd.graph import BatchGraph
    ds = SyntheticCellGraphs(5, 700, 4, base_seed=31, spatial=ordered)
    b = Batch.from_data_list([ds[i] for i in range(5)])
    assert bool(getattr(b, '_spatial', False)) == ordered
    gr = BatchGraph.from_batch(b.to(DEV), 0.4 if weighted else None)
    n = gr.n
    x = rnd(n, width, seed=3)
    post = rnd(n, seed=4).abs() + 0.5
    xb = torch.full((n, ld), 7.0, device=DEV)
    xb[:, :width] = g(x)
    visit = 1 | (4 if ordered else 0)
    for rowptr, col, val, pst in ((gr.rowptr, gr.col, gr.val, None), (gr.t_rowptr, gr.t_col, gr.t_val, g(post))):
        want = torch.zeros(n, width)
        REF.spmm(rowptr.cpu(), col.cpu(), None, None if val is None else val.cpu(), None, None if pst is None else pst.cpu(), x, want, n, width)
        ob = torch.full((n, ld), -3.0, device=DEV)
        hip().spmm(rowptr, col, None, val, None, pst, xb[:, :width], ob[:, :width], n, width, gr.gptr, gr.B, gr.nmax, visit, ld)
        close(ob[:, :width], want, what='wide spmm visit %d' % visit)
        assert bool((ob[:, width:] == -3.0).all())


GEMM_CASES = [
    # (M, N, K, tA, tB)
    (300, 200, 150, False, False), (129, 257, 33, False, True), (260, 140, 1000, True, False),
    (57, 20, 16, False, False), (1000, 60, 20, False, False), (20, 300, 900, True, False),
    (64, 1140, 20, False, False), (33, 114, 154, False, True), (500, 18, 18, False, True),
    (128, 128, 32, False, False), (1, 1, 1, False, False), (200, 130, 0, False, False),
]


@pytest.mark.parametrize('M,N,K,tA,tB', GEMM_CASES)
def test_gemm_flat(M, N, K, tA, tB):
    A = rnd(*((K, M) if tA else (M, K)), seed=1) if K > 0 else torch.zeros((0, M) if tA else (M, 0))
    B = rnd(*((N, K) if tB else (K, N)), seed=2) if K > 0 else torch.zeros((N, 0) if tB else (0, N))
    bias = rnd(N, seed=3)
    for alpha, beta, bi in ((1.0, 0.0, None), (0.5, 1.0, bias), (1.0, -2.0, None)):
        C0 = rnd(M, N, seed=4)
        want, got = C0.clone(), g(C0.clone())
        lda, ldb = max(A.shape[1], 1), max(B.shape[1], 1)
        REF.gemm(A, B, want, M, N, K, tA, tB, lda, ldb, N, alpha, beta, bi)
        hip().gemm(g(A) if A.numel() else got, g(B) if B.numel() else got, got, M, N, K, tA, tB, lda, ldb, N, alpha, beta, g(bi))
        close(got, want, 2e-5, 'gemm %s' % ((M, N, K, tA, tB, alpha, beta),))


def test_gemm_leading_dimensions_and_unaligned_views():
    # operands that are column slices of wider buffers (ld > width), including a 4-byte-misaligned start
    big_a, big_b, big_c = rnd(90, 77, seed=1), rnd(70, 95, seed=2), rnd(90, 101, seed=3)
    A, B = big_a[:, 3:3 + 50], big_b[:50, 5:5 + 61]          # [90,50] ld 77 ; [50,61] ld 95
    want = big_c.clone()
    ga, gb, gc = g(big_a), g(big_b), g(big_c.clone())
    REF.gemm(A, B, want[:, 7:], 90, 61, 50, False, False, 77, 95, 101, 1.0, 1.0)
    hip().gemm(ga[:, 3:], gb[:, 5:], gc[:, 7:], 90, 61, 50, False, False, 77, 95, 101, 1.0, 1.0)
    close(gc, want, 2e-5, 'gemm with lds')


SKINNY_CASES = [
    # (rows per batch item, batch, N, K, tB, ragged)   -- the step's thin products at their real sizes
    (16500, 1, 20, 1140, False, False), (16500, 1, 40, 1140, False, False), (16411, 1, 20, 1140, True, False),
    (1140, 16, 114, 1140, False, False), (1140, 16, 40, 1140, False, False), (1100, 16, 128, 516, True, False),
    (2153, 12, 20, 1140, False, True), (2153, 12, 100, 1140, True, True),
]


@pytest.mark.parametrize('rows,batch,N,K,tB,ragged', SKINNY_CASES)
def test_gemm_skinny_products(rows, batch, N, K, tB, ragged):
    """C = A op(B) with N <= 128 and a long K (S dX', dz W_narrow^T, A2 [h_e | h_p], A2 S2) on the 128x32 / 64x64 / 128x64
    tile shapes gemm_dispatch picks for them -- flat, strided batches and ragged-M batches (a B per graph), bias, K with a
    partial last k tile -- against fp64."""
    rng = np.random.RandomState(rows + N)
    if ragged:
        counts = rng.randint(rows // 2, rows + 1, size=batch)
        counts[0], counts[1] = rows, 1
        gptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
        n = int(counts.sum())
        A = rnd(n, K, seed=1)
        Bm = rnd(batch, *((N, K) if tB else (K, N)), seed=2)
        got = torch.full((n, N), float('nan'), device=DEV)
        hip().gemm(g(A), g(Bm), got, 0, N, K, False, tB, K, Bm.shape[2], N, 1.0, 0.0, None, batch, 0, K * N, 0, g(gptr), 1, rows, n)
        want = torch.cat([A[gptr[b]:gptr[b + 1]].double() @ (Bm[b].double().t() if tB else Bm[b].double()) for b in range(batch)])
    else:
        A = rnd(batch, rows, K, seed=1)
        Bm = rnd(batch, *((N, K) if tB else (K, N)), seed=2)
        bias = rnd(N, seed=3)
        got = torch.full((batch, rows, N), float('nan'), device=DEV)
        hip().gemm(g(A), g(Bm), got, rows, N, K, False, tB, K, Bm.shape[2], N, 0.5, 0.0, g(bias), batch, rows * K, Bm.shape[1] * Bm.shape[2],
                   rows * N)
        want = 0.5 * torch.bmm(A.double(), Bm.double().transpose(1, 2) if tB else Bm.double()) + bias.double()
    err = float((got.double().cpu() - want).abs().max() / want.abs().max())
    assert err < 2e-6, err


@pytest.mark.parametrize('tA,tB', [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize('M,N,K', [(1140, 114, 1140), (1140, 1140, 114), (114, 114, 1140), (250, 114, 70), (114, 30, 114)])
def test_gemm_odd_extents_on_padded_rows(M, N, K, tA, tB):
    """Extents that are not multiples of 4 (the level-2 cluster count 114) on rows padded to a multiple of 4 floats: the
    unguarded 16-byte loaders read into the padding, which must not reach any stored value -- the padding holds NaN here."""
    batch = 3
    pad = lambda w: (w + 3) // 4 * 4

    def padded(rows, cols, seed):
        full = torch.full((batch, rows, pad(cols)), float('nan'))
        full[:, :, :cols] = rnd(batch, rows, cols, seed=seed)
        return full
    A = padded(K, M, 1) if tA else padded(M, K, 1)
    Bm = padded(N, K, 2) if tB else padded(K, N, 2)
    C = torch.full((batch, M, pad(N)), float('nan'))
    gA, gB, gC = g(A), g(Bm), g(C)
    hip().gemm(gA, gB, gC, M, N, K, tA, tB, A.shape[2], Bm.shape[2], C.shape[2], 1.0, 0.0, None, batch,
               A.shape[1] * A.shape[2], Bm.shape[1] * Bm.shape[2], M * C.shape[2])
    a = A[:, :, :M].transpose(1, 2) if tA else A[:, :, :K]
    b = Bm[:, :, :K].transpose(1, 2) if tB else Bm[:, :, :N]
    want = torch.bmm(a.double(), b.double())
    got = gC.cpu()
    assert torch.isnan(got[:, :, N:]).all()                  # the padding of C is not written
    err = float((got[:, :, :N].double() - want).abs().max() / want.abs().max())
    assert err < 2e-6, err


@pytest.mark.parametrize('C,D', [(16, 8), (60, 60), (180, 60), (1140, 20)])
def test_gemm_ragged(C, D):
    counts = [37, 0, 130, 64, 201]
    n = sum(counts)
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    B_, nmax = len(counts), max(counts)
    S, X = rnd(n, C, seed=1), rnd(n, D, seed=2)
    # ragged K:  out[b] = S_b^T X_b
    want, got = torch.zeros(B_, C, D), torch.full((B_, C, D), 7.0, device=DEV)
    REF.gemm(S, X, want, C, D, 0, True, False, C, D, D, 1.0, 0.0, None, B_, 0, 0, C * D, gptr, 2, nmax)
    hip().gemm(g(S), g(X), got, C, D, 0, True, False, C, D, D, 1.0, 0.0, None, B_, 0, 0, C * D, g(gptr), 2, nmax)
    close(got, want, 2e-5, 'ragged-K')
    # ragged M:  Y_b = S_b G_b  (NN) and Z_b += X_b H_b^T (NT, beta=1)
    G = rnd(B_, C, D, seed=3)
    want, got = torch.zeros(n, D), torch.zeros(n, D, device=DEV)
    REF.gemm(S, G, want, 0, D, C, False, False, C, D, D, 1.0, 0.0, None, B_, 0, C * D, 0, gptr, 1, nmax)
    hip().gemm(g(S), g(G), got, 0, D, C, False, False, C, D, D, 1.0, 0.0, None, B_, 0, C * D, 0, g(gptr), 1, nmax)
    close(got, want, 2e-5, 'ragged-M NN')
    Z0 = rnd(n, C, seed=5)
    want, got = Z0.clone(), g(Z0.clone())
    REF.gemm(X, G, want, 0, C, D, False, True, D, D, C, 1.0, 1.0, None, B_, 0, C * D, 0, gptr, 1, nmax)
    hip().gemm(g(X), g(G), got, 0, C, D, False, True, D, D, C, 1.0, 1.0, None, B_, 0, C * D, 0, g(gptr), 1, nmax)
    close(got, want, 2e-5, 'ragged-M NT')


@pytest.mark.parametrize('nb', [8, 16, 24])
def test_gemm_ragged_balanced_dealing(nb):
    """Batches whose size is a multiple of 8 take the XCD-balanced tile dealing (gemm_map_tile: compact tile list for ragged
    M, serpentine by reduction length for ragged K): every tile must still be computed exactly once."""
    rng = np.random.RandomState(nb)
    counts = [int(c) for c in rng.randint(0, 300, size=nb)]
    counts[3] = 0
    n = sum(counts)
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    C, D, nmax = 150, 140, max(counts)
    S, X = rnd(n, C, seed=1), rnd(n, D, seed=2)
    want, got = torch.zeros(nb, C, D), torch.full((nb, C, D), 7.0, device=DEV)
    REF.gemm(S, X, want, C, D, 0, True, False, C, D, D, 1.0, 0.0, None, nb, 0, 0, C * D, gptr, 2, nmax)
    hip().gemm(g(S), g(X), got, C, D, 0, True, False, C, D, D, 1.0, 0.0, None, nb, 0, 0, C * D, g(gptr), 2, nmax)
    close(got, want, 2e-5, 'ragged-K')
    G = rnd(nb, C, D, seed=3)
    want, got = torch.zeros(n, D), torch.full((n, D), 7.0, device=DEV)
    REF.gemm(S, G, want, 0, D, C, False, False, C, D, D, 1.0, 0.0, None, nb, 0, C * D, 0, gptr, 1, nmax)
    hip().gemm(g(S), g(G), got, 0, D, C, False, False, C, D, D, 1.0, 0.0, None, nb, 0, C * D, 0, g(gptr), 1, nmax)
    close(got, want, 2e-5, 'ragged-M NN')


def test_gemm_extra_k_segments():
    """concatenated-K products without the concatenation: flat NT (Linear over cat) and ragged-M NT (dS += X dX'^T)."""
    n, fo = 333, 150
    x3, x12, W = rnd(n, 1140 // 10 * 4, seed=1), rnd(n, 40, seed=2), rnd(fo, 40 + 456, seed=3)
    bias = rnd(fo, seed=4)
    want = torch.cat([x12, x3], 1) @ W.t() + bias
    got = torch.empty(n, fo, device=DEV)
    gW = g(W)
    hip().gemm(g(x3), gW[:, 40:], got, n, fo, 456, False, True, 456, 496, fo, 1.0, 0.0, g(bias),
               extra=[(g(x12), gW, 40, 496, 40, 0, 0)])
    close(got, want, 2e-5, 'linear over cat')
    ref = torch.empty(n, fo)
    REF.gemm(x3, W[:, 40:], ref, n, fo, 456, False, True, 456, 496, fo, 1.0, 0.0, bias, extra=[(x12, W, 40, 496, 40, 0, 0)])
    close(ref, want, 2e-5, 'torch twin of the same call')
    counts = [37, 0, 130, 64, 201]
    nn_, C, D = sum(counts), 180, 60
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    P, X, dA, dX, Z0 = rnd(nn_, C, seed=5), rnd(nn_, D, seed=6), rnd(5, C, C, seed=7), rnd(5, C, D, seed=8), rnd(nn_, C, seed=9)
    want, got = Z0.clone(), g(Z0.clone())
    args = (0, C, C, False, True, C, C, C, 1.0, 1.0, None, 5, 0, C * C, 0)
    REF.gemm(P, dA, want, *args, gptr, 1, max(counts), nn_, extra=[(X, dX, D, D, D, 0, C * D)])
    hip().gemm(g(P), g(dA), got, *args, g(gptr), 1, max(counts), nn_, extra=[(g(X), g(dX), D, D, D, 0, C * D)])
    close(got, want, 2e-5, 'ragged-M with an extra segment')
    manual = Z0.clone()
    for b in range(5):
        lo, hi = int(gptr[b]), int(gptr[b + 1])
        manual[lo:hi] += P[lo:hi] @ dA[b].t() + X[lo:hi] @ dX[b].t()
    close(want, manual, 2e-5, 'twin vs explicit formula')


@pytest.mark.parametrize('cfg', [12, 13, 14, 15, 16])
@pytest.mark.parametrize('tA,tB', [(False, False), (True, False), (False, True)])
def test_gemm_small_tiles_split_when_underfilled(cfg, tA, tB):
    """The smaller pipelined tile shapes (128x64, 64x128, 64x64, 128x32, 32x128) cut the tiles of an under-filled launch along K as
    the 128 x 128 kernel does for its tail (the thin level-2 products of a small shard).  Against fp64, against the unsplit launch,
    bitwise repeatable; beta / bias through the fix-up's epilogue; N = 40 leaves a ragged column tile."""
    k = hip()
    old = k.lib.cgc_gemm_tuning(cfg)
    try:
        batch, M, N, K = 3, 333, 40, 1140
        A = rnd(batch, *((K, M) if tA else (M, K)), seed=1)
        B = rnd(batch, *((N, K) if tB else (K, N)), seed=2)
        C0, bias = rnd(batch, M, N, seed=3), rnd(N, seed=4)
        want = torch.bmm(A.double().transpose(1, 2) if tA else A.double(), B.double().transpose(1, 2) if tB else B.double())
        want = want + 0.5 * C0.double() + bias.double()
        gA, gB = g(A), g(B)
        lda, ldb = A.shape[2], B.shape[2]
        outs = []
        for split in (True, True, False):
            k.tail_split = split
            got = g(C0.clone())
            k.gemm(gA, gB, got, M, N, K, tA, tB, lda, ldb, N, 1.0, 0.5, g(bias), batch, A.shape[1] * lda, B.shape[1] * ldb, M * N)
            outs.append(got.cpu())
    finally:
        k.tail_split = True
        k.lib.cgc_gemm_tuning(old)
    assert torch.equal(outs[0], outs[1])
    scale = float(want.abs().max())
    for o in (outs[0], outs[2]):
        assert float((o.double() - want).abs().max()) <= 2e-5 * scale
    assert float((outs[0] - outs[2]).abs().max()) <= 1e-5 * scale


TAIL_CASES = [
    # (M or rows/graph list, N, K, tA, tB, batch, ragged)  -- with the 128 x 128 pipelined kernel forced (cgc_gemm_tuning(11))
    (1000, 700, 500, False, False, 1, 0),        # 48 tiles < 512: every tile is a tail tile, 5 pieces
    (1000, 700, 500, False, True, 1, 0),
    (900, 1140, 1000, True, False, 1, 0),
    (3840, 2304, 200, False, True, 1, 0),        # 540 tiles: 512 whole + 28 tail tiles in 2 pieces
    (700, 600, 333, False, False, 7, 0),         # strided batch, 210 tiles, K not a multiple of the k-tile
    ([300, 0, 513, 128, 77, 900, 250, 640], 520, 400, False, False, 8, 1),   # ragged M, compact list (batch % 8 == 0)
    ([300, 0, 513, 128, 77], 520, 400, False, True, 5, 1),                    # ragged M, plain cut (empty tiles in the tail)
    ([300, 0, 513, 128, 77, 900, 250, 640], 520, 0, True, False, 8, 2),      # ragged K, serpentine dealing
    ([300, 0, 513], 520, 0, True, False, 3, 2),                               # ragged K, plain cut; one empty reduction
    (1140, 1140, 1800, True, False, 4, 0),       # 324 tiles of 57 k-tiles (S^T P of a 4-graph shard): every tile in 2 pieces
    ([1800, 1900, 1750, 1860, 1700, 1650, 2000, 1810], 1140, 0, True, False, 8, 2),   # 288 ragged-K tiles in 2 pieces, serpentine dealing
]


@pytest.mark.parametrize('rows,N,K,tA,tB,batch,ragged', TAIL_CASES)
def test_gemm_tail_split(rows, N, K, tA, tB, batch, ragged):
    """The tail split of the 128 x 128 kernel (include/cgc_hip.h: cgc_gemm_f32): tiles of the last partial round cut along K
    into pieces + slab fix-up.  Against fp64, against the unsplit launch (same arithmetic per element up to the order of the
    K pieces), and bitwise repeatable; alpha / beta / bias / an extra K segment go through the fix-up's epilogue."""
    k = hip()
    old = k.lib.cgc_gemm_tuning(11)
    try:
        if ragged == 0:
            M = rows
            A = rnd(batch, *((K, M) if tA else (M, K)), seed=1)
            B = rnd(batch, *((N, K) if tB else (K, N)), seed=2)
            want = torch.bmm(A.double().transpose(1, 2) if tA else A.double(), B.double().transpose(1, 2) if tB else B.double())
            C0 = rnd(batch, M, N, seed=3)
            bias = rnd(N, seed=4)
            want = 0.5 * want + 2.0 * C0.double() + bias.double()
            gA, gB = g(A), g(B)
            lda, ldb = A.shape[2], B.shape[2]
            args = (M, N, K, tA, tB, lda, ldb, N, 0.5, 2.0, g(bias), batch, A.shape[1] * lda, B.shape[1] * ldb, M * N)
            outs = []
            for split in (True, True, False):
                k.tail_split = split
                got = g(C0.clone())
                k.gemm(gA, gB, got, *args)
                outs.append(got.cpu())
        else:
            counts = rows
            n, nmax = sum(counts), max(counts)
            gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
            C = 450
            if ragged == 1:          # Y_b = S_b op(G_b) + X_b op(H_b) (extra K segment), rows of graph b
                S, X = rnd(n, K, seed=1), rnd(n, 60, seed=5)
                G = rnd(batch, *((N, K) if tB else (K, N)), seed=2)
                H = rnd(batch, *((N, 60) if tB else (60, N)), seed=6)
                want = torch.cat([S[gptr[b]:gptr[b + 1]].double() @ (G[b].double().t() if tB else G[b].double()) +
                                  X[gptr[b]:gptr[b + 1]].double() @ (H[b].double().t() if tB else H[b].double())
                                  for b in range(batch)])
                C0 = rnd(n, N, seed=3)
                want = want + C0.double()
                gS, gG, gX, gH, gp = g(S), g(G), g(X), g(H), g(gptr)
                outs = []
                for split in (True, True, False):
                    k.tail_split = split
                    got = g(C0.clone())
                    k.gemm(gS, gG, got, 0, N, K, False, tB, K, G.shape[2], N, 1.0, 1.0, None, batch, 0, G.shape[1] * G.shape[2], 0,
                           gp, 1, nmax, n, extra=[(gX, gH, 60, H.shape[2], 60, 0, H.shape[1] * H.shape[2])])
                    outs.append(got.cpu())
            else:                    # out[b] = S_b^T X_b, reduction over the rows of graph b
                S, X = rnd(n, C, seed=1), rnd(n, N, seed=2)
                want = torch.stack([S[gptr[b]:gptr[b + 1]].double().t() @ X[gptr[b]:gptr[b + 1]].double() for b in range(batch)])
                gS, gX, gp = g(S), g(X), g(gptr)
                outs = []
                for split in (True, True, False):
                    k.tail_split = split
                    got = torch.full((batch, C, N), 7.0, device=DEV)
                    k.gemm(gS, gX, got, C, N, 0, True, False, C, N, N, 1.0, 0.0, None, batch, 0, 0, C * N, gp, 2, nmax, n)
                    outs.append(got.cpu())
    finally:
        k.tail_split = True
        k.lib.cgc_gemm_tuning(old)
    assert torch.equal(outs[0], outs[1])                                   # fixed summation order: bitwise repeatable
    scale = float(want.abs().max())
    for o, what in zip((outs[0], outs[2]), ('split', 'whole')):
        assert float((o.double() - want.reshape(o.shape)).abs().max()) < 1e-5 * scale, what
    assert float((outs[0].double() - outs[2].double()).abs().max()) < 1e-5 * scale


def test_gemm_strided_batch_and_splitk_reduce():
    A, B = rnd(5, 70, 90, seed=1), rnd(5, 90, 40, seed=2)
    want, got = torch.zeros(5, 70, 40), torch.zeros(5, 70, 40, device=DEV)
    REF.gemm(A, B, want, 70, 40, 90, False, False, 90, 40, 40, 1.0, 0.0, None, 5, 70 * 90, 90 * 40, 70 * 40)
    hip().gemm(g(A), g(B), got, 70, 40, 90, False, False, 90, 40, 40, 1.0, 0.0, None, 5, 70 * 90, 90 * 40, 70 * 40)
    close(got, want, 2e-5, 'strided batch')
    ws = rnd(6, 1234, seed=3)
    o0 = rnd(1234, seed=4)
    for beta in (0.0, 1.0):
        want, got = o0.clone(), g(o0.clone())
        REF.reduce_batch_sum(ws, want, 6, 1234, beta)
        hip().reduce_batch_sum(g(ws), got, 6, 1234, beta)
        close(got, want, 1e-6, 'reduce_batch_sum')


SHAPES = [(50, 8), (333, 20), (257, 18), (100, 60), (90, 114), (70, 180), (64, 250), (300, 1140), (40, 1600), (33, 2047)]


@pytest.mark.parametrize('n,F', SHAPES)
@pytest.mark.parametrize('act', [1, 2, 3])
def test_conv_epilogue_chain(n, F, act):
    k = hip()
    h = rnd(n, F, seed=F)
    h[min(3, n - 1)] = 0.0                      # a zero row: the 1e-12 clamp of F.normalize
    count = float(n + 17)                       # BatchNorm sees 17 extra zero rows (padding of the dense layout)
    gamma, beta = rnd(F, seed=1).abs() + 0.5, rnd(F, seed=2)
    outs = {}
    for name, K_, dev in (('ref', REF, 'cpu'), ('hip', k, DEV)):
        t = lambda v: v.to(dev)
        hn, rinv = torch.empty(n, F, device=dev), torch.empty(n, device=dev)
        stats = torch.empty(2, F, device=dev, dtype=torch.float64)
        K_.l2norm_act_stats(t(h), n, F, True, act, hn, rinv, stats)
        rm, rv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        mean, istd = torch.empty(F, device=dev), torch.empty(F, device=dev)
        K_.bn_finalize(stats, count, 1e-5, 0.1, rm, rv, mean, istd)
        y = torch.zeros(n, F + 4, device=dev)                  # write into a column slice of a wider buffer
        K_.bn_act_apply(hn, n, F, act, mean, istd, t(gamma), t(beta), y, F + 4)
        dy_big = t(rnd(n, F + 8, seed=9))
        dy = dy_big[:, 4:4 + F]                                  # strided incoming gradient (slice of a cat grad)
        sums = torch.empty(2, F, device=dev)
        K_.bn_bwd_reduce(dy, F + 8, hn, n, F, act, mean, istd, sums)
        dh = torch.empty(n, F, device=dev)
        dhc = torch.empty(F, device=dev)                        # fused column sums of dh (bias gradient)
        K_.bn_act_l2_bwd(dy, F + 8, hn, rinv, n, F, act, True, 2, mean, istd, t(gamma), sums, count, dh, dhc)
        dh1 = torch.empty(n, F, device=dev)
        K_.bn_act_l2_bwd(dy, F + 8, hn, rinv, n, F, act, False, 1, mean, istd, t(gamma), sums, count, dh1)
        cs = torch.empty(F, device=dev)
        K_.colsum(dy, F + 8, n, F, cs)
        mask_ = torch.ones(n, dtype=torch.bool, device=dev)
        mask_[min(3, n - 1)] = False                             # the clamped zero row carries a 1e12 factor: compare without it
        outs[name] = dict(hn=hn, rinv=rinv, stats=stats, rm=rm, rv=rv, mean=mean, istd=istd, y=y, sums=sums, dh=dh,
                          dh1=dh1, cs=cs, dhc_consistent=(dhc - dh[~mask_].sum(0)), dh_colsum=dh[mask_].sum(0))
    torch.cuda.synchronize()
    for key in outs['ref']:
        tol = 1e-3 if key in ('dh',) and h[min(3, n - 1)].abs().sum() == 0 else TOL
        a, b = outs['hip'][key], outs['ref'][key]
        if key in ('dh', 'hn', 'rinv'):                          # exclude the clamped zero row's 1e12 factor from the scale
            mask = torch.ones(n, dtype=torch.bool)
            mask[min(3, n - 1)] = False
            close(a.cpu()[mask], b[mask], TOL, key)
            close(a.cpu()[~mask], b[~mask], 1e-3, key + ' (clamped row)')
        else:
            close(a, b, tol, key)


@pytest.mark.parametrize('n,F', [(50, 8), (333, 20), (5000, 20), (4100, 60), (2000, 128), (300, 1140), (1, 16)])
def test_fused_statistics_and_finalize(n, F):
    """cgc_l2norm_act_bn = l2norm_act_stats + bn_finalize + num_batches_tracked += 1 behind one entry point."""
    k = hip()
    count = float(n + 23)
    res = {}
    for name, K_, dev in (('ref', REF, 'cpu'), ('hip', k, DEV)):
        rm, rv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        outs = []
        for rep in range(3):
            h = rnd(n, F, seed=F + rep).to(dev)
            hn, rinv = torch.empty(n, F, device=dev), torch.empty(n, device=dev)
            mean, istd = torch.empty(F, device=dev), torch.empty(F, device=dev)
            K_.l2norm_act_bn(h, n, F, True, 1, hn, rinv, count, 1e-5, 0.1, rm, rv, nbt, mean, istd)
            outs += [hn, rinv, mean, istd]
        res[name] = outs + [rm, rv, nbt.double()]
    torch.cuda.synchronize()
    assert int(res['hip'][-1].item()) == 3
    for a, b in zip(res['hip'], res['ref']):
        close(a, b)


@pytest.mark.parametrize('n,K_,F,lda', [(1, 20, 256, 20), (37, 20, 1140, 40), (1000, 16, 1600, 16), (4100, 20, 1140, 40), (300, 7, 257, 12),
                                         (50, 32, 200, 32), (50, 20, 1700, 20), (50, 33, 512, 36),
                                         (1000, 20, 20, 40), (37, 16, 20, 16), (5, 32, 32, 32), (4100, 20, 18, 20), (1, 8, 4, 8),
                                         # >= 12288 rows: the quadratic-form row norms + one wave per 32 x 96 block (k_sage_wide_cols)
                                         (12301, 20, 1140, 40), (13000, 16, 1600, 16), (12800, 21, 320, 24), (12290, 7, 257, 12)])
@pytest.mark.parametrize('stats,act', [(True, 1), (False, 1), (True, 2), (True, 3), (False, 0)])
def test_fused_wide_sage_forward(n, K_, F, lda, stats, act):
    """cgc_sage_wide_fwd: rank-K projection + bias + L2 normalisation (+ BatchNorm statistics, running stats, batch counter) in one
    matrix-core kernel, against GEMM + l2norm_act_bn of the contract; shapes outside its envelope report False and touch nothing."""
    k = hip()
    big = rnd(n, lda + 4, seed=n)
    W, bias = rnd(K_, F, seed=1), rnd(F, seed=2)
    count = float(n + 11)
    res = {}
    for name, K__, dev in (('ref', REF, 'cpu'), ('hip', k, DEV)):
        agg = big.to(dev)[:, 4:4 + lda]                          # a column window of a wider buffer (row stride lda + 4)
        hn, rinv = torch.full((n, F), 7.0, device=dev), torch.empty(n, device=dev)
        rm, rv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        nbt = torch.zeros((), dtype=torch.int64, device=dev)
        mean, istd = torch.zeros(F, device=dev), torch.zeros(F, device=dev)
        ok = K__.sage_wide_fwd(agg, lda + 4, W.to(dev), bias.to(dev), n, K_, F, True, act, hn, rinv, stats, count, 1e-5, 0.1,
                               rm if stats else None, rv if stats else None, nbt if stats else None,
                               mean if stats else None, istd if stats else None)
        res[name] = (ok, hn, rinv, rm, rv, mean, istd, nbt.double())
    torch.cuda.synchronize()
    assert res['hip'][0] == res['ref'][0] == (K_ <= 32 and F <= 1664)
    if not res['hip'][0]:
        assert float(res['hip'][1].min()) == 7.0                 # untouched
        return
    for i in range(1, 8):
        close(res['hip'][i], res['ref'][i], TOL, 'sage_wide %d' % i)


@pytest.mark.parametrize('n,F', [(1000, 200), (4100, 1140), (97, 1140), (65, 33), (12301, 1140), (20011, 264)])
def test_fused_wide_sage_forward_writes_nothing_past_its_rows(n, F):
    """The partial last row tile of cgc_sage_wide_fwd (n % 32 != 0): the rows of the tile that lie past n must not be stored -- hn
    sits inside a larger canary-filled allocation here (in the step: the next arena region)."""
    k = hip()
    K_ = 20
    agg, W, bias = rnd(n, K_, seed=n).to(DEV), rnd(K_, F, seed=1).to(DEV), rnd(F, seed=2).to(DEV)
    big = torch.full((n + 40, F), 7.0, device=DEV)
    hn, rinv = big[:n], torch.empty(n, device=DEV)
    mean, istd = torch.zeros(F, device=DEV), torch.zeros(F, device=DEV)
    rm, rv, nbt = torch.zeros(F, device=DEV), torch.ones(F, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    assert k.sage_wide_fwd(agg, K_, W, bias, n, K_, F, True, 1, hn, rinv, True, float(n), 1e-5, 0.1, rm, rv, nbt, mean, istd)
    torch.cuda.synchronize()
    assert float(big[n:].min()) == 7.0 and float(big[n:].max()) == 7.0
    assert float((big[:n].norm(dim=1) - 1.0).abs().max()) < 1e-5          # the rows themselves were written (unit norm)


def test_wide_sage_row_norms_from_the_quadratic_form():
    """The large-launch route of cgc_sage_wide_fwd takes 1 / ||agg W + b|| from agg^T (W W^T) agg + 2 agg . (W b) + b . b in double
    (k_sage_gram + k_sage_rinv) instead of from the projected row: rows of very different scales, rows whose projection is zero
    (zero input under a zero bias: the reference's F.normalize divides by eps = 1e-12 and the row stays zero) and the no-bias form
    must give the float64 norm to float32 rounding, and unit rows."""
    k = hip()
    n, K_, F = 12288 + 77, 20, 1140
    g = torch.Generator().manual_seed(3)
    agg = torch.randn(n, K_, generator=g)
    agg[5] = 0.0
    agg[100:200] *= 1e3
    agg[200:300] *= 1e-3
    agg[n - 1] = 0.0
    W = torch.randn(K_, F, generator=g) * 0.2
    for bias in (torch.zeros(F), torch.randn(F, generator=g) * 0.1, None):
        hn, rinv = torch.full((n, F), 7.0, device=DEV), torch.empty(n, device=DEV)
        assert k.sage_wide_fwd(agg.to(DEV), K_, W.to(DEV), None if bias is None else bias.to(DEV), n, K_, F, True, 1, hn, rinv, False, float(n),
                               1e-5, 0.1, None, None, None, None, None)
        torch.cuda.synchronize()
        h = agg.double() @ W.double() + (0.0 if bias is None else bias.double())
        nrm = h.norm(dim=1)
        want = 1.0 / nrm.clamp_min(1e-12)
        assert float((rinv.double().cpu() / want - 1.0).abs().max()) < 3e-7
        ref = h / nrm.clamp_min(1e-12)[:, None]
        assert float((hn.double().cpu() - ref).abs().max()) < 2e-7
        zero = nrm == 0
        if bool(zero.any()):
            assert float(hn.cpu()[zero].abs().max()) == 0.0 and float(rinv.cpu()[zero].min()) == float(torch.tensor(1e12, dtype=torch.float32))


@pytest.mark.parametrize('n,fin,F', [(1, 20, 20), (37, 16, 20), (1000, 20, 20), (4100, 20, 18), (333, 8, 32), (64, 32, 8), (50, 20, 33)])
@pytest.mark.parametrize('mode,act,normalize', [(2, 1, True), (1, 3, True), (0, 2, False), (2, 2, True)])
def test_fused_narrow_sage_backward(n, fin, F, mode, act, normalize):
    """cgc_sage_narrow_bwd (BN / activation / L2 backward + d agg + d W + d b in one kernel, dh never written) against the
    composition bn_act_l2_bwd -> matmuls of the contract; strided dy / agg windows, a zero row (norm clamp), all BN modes.  With that
    row its 1e12 factor sets the scale of `dW | db` here: tests/test_sage_fp64_gpu.py pins them element by element without it."""
    k = hip()
    h = rnd(n, F, seed=n + F)
    h[min(3, n - 1)] = 0.0
    big_dy, big_agg = rnd(n, F + 8, seed=1), rnd(n, fin + 5, seed=2)
    W = rnd(fin, F, seed=3)
    gamma, count = rnd(F, seed=4).abs() + 0.5, float(n + 9)
    res = {}
    for name, K_, dev in (('ref', REF, 'cpu'), ('hip', k, DEV)):
        t = lambda v: v.to(dev)
        hn, rinv = torch.empty(n, F, device=dev), torch.empty(n, device=dev)
        stats = torch.empty(2, F, device=dev, dtype=torch.float64)
        K_.l2norm_act_stats(t(h), n, F, normalize, act, hn, rinv, stats)
        mean, istd = torch.empty(F, device=dev), torch.empty(F, device=dev)
        K_.bn_finalize(stats, count, 1e-5, 0.1, None, None, mean, istd)
        dy, agg = t(big_dy)[:, 4:4 + F], t(big_agg)[:, 5:5 + fin]
        sums = torch.zeros(2, F, device=dev)
        if mode == 2:
            K_.bn_bwd_reduce(dy, F + 8, hn, n, F, act, mean, istd, sums)
        dagg, dwdb = torch.full((n, fin), 7.0, device=dev), torch.full((fin * F + F,), 7.0, device=dev)
        ok = K_.sage_narrow_bwd(dy, F + 8, hn, rinv, n, F, act, normalize, mode, mean if mode else None, istd if mode else None,
                                t(gamma) if mode else None, sums if mode == 2 else None, count, agg, fin + 5, fin, t(W), dagg, dwdb)
        ok2 = K_.sage_narrow_bwd(dy, F + 8, hn, rinv, n, F, act, normalize, mode, mean if mode else None, istd if mode else None,
                                 t(gamma) if mode else None, sums if mode == 2 else None, count, agg, fin + 5, fin, t(W), None,
                                 torch.empty_like(dwdb))
        res[name] = (ok and ok2, dagg, dwdb)
    torch.cuda.synchronize()
    assert res['hip'][0] == res['ref'][0] == (F <= 32 and fin <= 32)
    if not res['hip'][0]:
        assert float(res['hip'][1].min()) == 7.0
        return
    mask = torch.ones(n, dtype=torch.bool)
    if normalize:
        mask[min(3, n - 1)] = False                 # the clamped zero row carries a 1e12 factor: compared on its own scale
    close(res['hip'][1].cpu()[mask], res['ref'][1][mask], TOL, 'dagg')
    close(res['hip'][1].cpu()[~mask], res['ref'][1][~mask], 1e-3, 'dagg (clamped row)')
    if bool(mask.all()) or not normalize:
        close(res['hip'][2], res['ref'][2], TOL, 'dW | db')
    else:
        close(res['hip'][2], res['ref'][2], 1e-3, 'dW | db (with the clamped row)')


def test_epilogue_without_bn_and_without_normalize():
    k = hip()
    n, F = 77, 20
    h = rnd(n, F)
    for normalize in (True, False):
        r = {}
        for name, K_, dev in (('ref', REF, 'cpu'), ('hip', k, DEV)):
            hn, rinv = torch.empty(n, F, device=dev), torch.empty(n, device=dev)
            K_.l2norm_act_stats(h.to(dev), n, F, normalize, 0, hn, rinv, None)
            y = torch.empty(n, F, device=dev)
            K_.bn_act_apply(hn, n, F, 1, None, None, None, None, y, F)
            dh = torch.empty(n, F, device=dev)
            K_.bn_act_l2_bwd(rnd(n, F, seed=3).to(dev), F, hn, rinv, n, F, 1, normalize, 0, None, None, None, None, 1.0, dh)
            r[name] = (hn, y, dh)
        for a, b in zip(r['hip'], r['ref']):
            close(a, b)


@pytest.mark.parametrize('n,C', [(40, 4), (100, 16), (37, 60), (64, 114), (50, 180), (200, 1140), (9, 1600)])
def test_softmax(n, C):
    x = rnd(n, C, seed=C) * 3
    want, got = torch.empty(n, C), torch.empty(n, C, device=DEV)
    REF.softmax_fwd(x, n, C, want)
    hip().softmax_fwd(g(x), n, C, got)
    close(got, want, 1e-5, 'softmax')
    dS = rnd(n, C, seed=1)
    w2, g2 = torch.empty(n, C), torch.empty(n, C, device=DEV)
    wc, gc = torch.empty(C), torch.empty(C, device=DEV)
    REF.softmax_bwd(want, dS, n, C, w2, wc)
    hip().softmax_bwd(g(want), g(dS), n, C, g2, gc)
    close(g2, w2, 1e-5, 'softmax bwd')
    close(gc, wc, 1e-4, 'softmax bwd fused column sums')
    g3 = torch.empty(n, C, device=DEV)
    hip().softmax_bwd(g(want), g(dS), n, C, g3)            # without the fused sums
    close(g3, w2, 1e-5, 'softmax bwd (no colsum)')
    inpl = g(x.clone())
    hip().softmax_fwd(inpl, n, C, inpl)                    # in-place forward (used by the fused Linear+softmax node)
    close(inpl, want, 1e-5, 'softmax in place')


@pytest.mark.parametrize('D', [8, 20, 60, 100])
def test_segment_max(D):
    counts = [17, 0, 300, 64, 5]
    n, B_ = sum(counts), len(counts)
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    x = rnd(n, D, seed=D)
    x[17:317, 0] = -1.0 - x[17:317, 0].abs()      # graph 2, column 0 all negative: the zero padding wins there
    x[20, 1] = x[30, 1] = 9.0                      # a tie: first index must win
    for nmax in (300, 400):                        # graph 2 is the longest (no padding) / everybody is padded
        want, warg = torch.empty(B_, D), torch.empty(B_, D, dtype=torch.int32)
        got, garg = torch.empty(B_, D, device=DEV), torch.empty(B_, D, dtype=torch.int32, device=DEV)
        REF.segment_max_fwd(x, gptr, B_, D, nmax, want, warg)
        hip().segment_max_fwd(g(x), g(gptr), B_, D, nmax, got, garg)
        assert torch.equal(got.cpu(), want) and torch.equal(garg.cpu(), warg)
        dout = rnd(B_, D, seed=1)
        wdx, gdx = torch.zeros(n, D), torch.zeros(n, D, device=DEV)
        REF.segment_max_bwd(dout, warg, B_, D, wdx)
        hip().segment_max_bwd(g(dout), garg, B_, D, gdx)
        assert torch.equal(gdx.cpu(), wdx)
        full = torch.full((n, D), float('nan'), device=DEV)          # the variant that needs no zero-filled buffer
        hip().segment_max_bwd_full(g(dout), garg, g(gptr), B_, D, nmax, full)
        assert torch.equal(full.cpu(), wdx)


@pytest.mark.parametrize('B_,C', [(3, 4), (2, 16), (3, 60), (2, 114), (2, 180), (1, 1140), (1, 1600)])
def test_dense_adjacency_transforms(B_, C):
    R = B_ * C
    A = rnd(B_, C, C, seed=C).abs()
    A[0, 1] *= 0.001                               # a row whose sum is < 1: clamp(min=1) active, ge1 = 0
    dO = rnd(B_, C, C, seed=1)
    res = {}
    for name, K_, dev in (('ref', REF, 'cpu'), ('hip', hip(), DEV)):
        a, d = A.to(dev), dO.to(dev)
        out, invd, ge1 = torch.empty_like(a), torch.empty(R, device=dev), torch.empty(R, device=dev)
        K_.dense_rownorm_fwd(a, R, C, out, invd, ge1)
        dA = torch.empty_like(a)
        K_.dense_rownorm_bwd(d, out, invd, ge1, R, C, dA)
        rn, drn = torch.empty_like(a), torch.empty_like(a)
        K_.dense_renorm_fwd(a, R, C, 0.4, rn)
        K_.dense_renorm_bwd(a, d, R, C, 0.4, drn)
        res[name] = (out, invd, ge1, dA, rn, drn)
    for i, (x, y) in enumerate(zip(res['hip'], res['ref'])):
        close(x, y, 2e-5, 'dense transform %d' % i)


@pytest.mark.parametrize('B_,C', [(3, 4), (2, 18), (3, 60), (2, 114), (1, 1140), (1, 1600)])
@pytest.mark.parametrize('p', [None, 0.4])
@pytest.mark.parametrize('second_stream', [False, True])
def test_fused_adjacency_preparation(B_, C, p, second_stream):
    """cgc_adj_prep_{fwd,bwd}: re-normalisation + clamped row normalisation in one pass, with the gradient that reaches the
    re-normalised adjacency directly (second_stream) folded into the backward -- against the composition of the unfused ops."""
    R = B_ * C
    A = rnd(B_, C, C, seed=C).abs()
    A[0, 1] *= 0.001
    gAn, gAt = rnd(B_, C, C, seed=1), (rnd(B_, C, C, seed=2) if second_stream else None)
    res = {}
    for name, K_, dev in (('ref', REF, 'cpu'), ('hip', hip(), DEV)):
        a = A.to(dev)
        At = torch.empty_like(a) if p is not None else None
        An, invd, ge1 = torch.empty_like(a), torch.empty(R, device=dev), torch.empty(R, device=dev)
        K_.adj_prep_fwd(a, R, C, p, At, An, invd, ge1)
        dA = torch.empty_like(a)
        K_.adj_prep_bwd(a, An, invd, ge1, gAn.to(dev), None if gAt is None else gAt.to(dev), R, C, p, dA)
        res[name] = ([At] if At is not None else []) + [An, invd, dA]
    for i, (x, y) in enumerate(zip(res['hip'], res['ref'])):
        close(x, y, 2e-5, 'adj_prep %d' % i)


@pytest.mark.parametrize('C,n', [(8, 37), (20, 300), (16, 1500), (20, 2500), (4, 200), (12, 700), (6, 130), (24, 300), (32, 257),
                                 (20, 20011), (8, 9001)])        # (more 32-node tiles than persistent workgroups: 626 / 282 for 256)
def test_dense_jk_kernels(C, n):
    """Fused bi-LSTM + attention (csrc/jk.hip, csrc/jk_mfma.hip) against the torch restatement, and that restatement against
    torch.nn.LSTM.  Every even channel count up to 32 is compiled in (--hidden-dim of train.py): C in 4/8/12/16/20 on the matrix-core
    kernels, the rest on the thread-per-direction kernels with staged parameter gradients."""
    assert hip().jk_supported(C)
    H = 3 * C // 2
    torch.manual_seed(C + n)
    lstm_mod = torch.nn.LSTM(C, H, bidirectional=True, batch_first=True)
    att = torch.nn.Linear(2 * H, 1)
    xs = torch.randn(n, 3 * C)
    p = lstm_mod
    lstm = [t.detach() for t in (p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, p.weight_ih_l0_reverse,
                                 p.weight_hh_l0_reverse, p.bias_ih_l0_reverse, p.bias_hh_l0_reverse)]
    w_att, b_att = att.weight.detach().reshape(-1), att.bias.detach()
    npad = -(-n // 1024) * 1024
    # torch.nn.LSTM semantics of the twin (pins the gate order / direction handling)
    seq = xs.reshape(n, 3, C)
    alpha, _ = lstm_mod(seq)
    a = torch.softmax(att(alpha).squeeze(-1), dim=-1)
    want_out = (seq * a.unsqueeze(-1)).sum(1).detach()
    res = {}
    for name, K_, dev in (('ref', REF, 'cpu'), ('hip', hip(), DEV)):
        t = lambda v: v.to(dev)
        out = torch.empty(n, C, device=dev)
        HS, CS = torch.zeros(6 * H, npad, device=dev), torch.zeros(6 * H, npad, device=dev)
        K_.jk_fwd(t(xs), n, npad, C, [t(v) for v in lstm], t(w_att), t(b_att), out, HS, CS)
        dout = t(rnd(n, C, seed=3))
        dxs = torch.empty(n, 3 * C, device=dev)
        DGT = torch.full((2, 4 * H + 1, 3 * npad), 7.0, device=dev)
        INT = torch.full((2, C + 2 * H + 1, 3 * npad), 7.0, device=dev)
        DHC = torch.empty(2, 2, H, npad, device=dev)
        K_.jk_bwd(t(xs), dout, n, npad, C, [t(v) for v in lstm], t(w_att), t(b_att), HS, CS, dxs, DGT, INT, DHC)
        G = torch.stack([DGT[d].double().cpu() @ INT[d].double().cpu().t() for d in range(2)])
        # the same backward with the parameter gradients accumulated in-kernel
        dxs2 = torch.empty(n, 3 * C, device=dev)
        G2 = torch.full((2, 4 * H + 1, C + 2 * H + 1), 7.0, device=dev)
        K_.jk_bwd_params(t(xs), dout, n, npad, C, [t(v) for v in lstm], t(w_att), t(b_att), HS, CS, dxs2, G2)
        G2 = G2.double().cpu()
        for g_ in (G, G2):
            g_[:, :4 * H, C + H + 1:] = 0       # unused corner blocks of the factorisation
            g_[:, 4 * H, :C + H] = 0
            g_[1, 4 * H, C + H] = 0
        res[name] = dict(out=out, HS=HS[:, :n], CS=CS[:, :n], dxs=dxs, G=G, dxs2=dxs2, G2=G2)
    close(res['ref']['out'], want_out, 1e-5, 'twin vs torch.nn.LSTM')
    for k in res['ref']:
        close(res['hip'][k], res['ref'][k], 2e-4 if k in ('G', 'G2') else 2e-5, 'jk ' + k)


# ------------------------------------------------------------------ F2: cell-graph construction (radius k-NN)
def _rows_as_sets(ei, n):
    rows = [[] for _ in range(n)]
    for r_, c_ in zip(ei[0].tolist(), ei[1].tolist()):
        rows[r_].append(c_)
    return rows


@pytest.mark.parametrize('counts,side,k,loop', [([300], 700.0, 8, True), ([1800, 1500, 2100], 1800.0, 8, True),
                                                ([257, 1, 0, 64, 5], 300.0, 8, True), ([400, 380], 900.0, 8, False),
                                                ([500], 900.0, 16, True), ([200, 200], 4000.0, 4, True)])
def test_radius_knn_matches_the_host_tree(counts, side, k, loop):
    """csrc/knn.hip against cKDTree.query(k+1, r+1e-8) per graph (the reference's torch_cluster CPU path)."""
    rng = np.random.RandomState(sum(counts) + k)
    n = sum(counts)
    pos = torch.from_numpy(rng.uniform(0.0, side, size=(n, 2)).astype(np.float32))
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    want = REF.radius_knn(pos, gptr, len(counts), 100.0, k, loop)
    got = hip().radius_knn(g(pos), g(gptr), len(counts), 100.0, k, loop).cpu()
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got[0], want[0])                              # same degree per node, rows ascending
    # neighbour order: by distance; compare as ordered lists (random positions: no distance ties)
    assert torch.equal(got[1], want[1])


def test_radius_knn_degenerate_layouts():
    """Coincident points, a single line of points, and a far-away cluster (huge bounding box) stay exact and bounded."""
    rng = np.random.RandomState(3)
    line = np.stack([np.linspace(0, 5.0e5, 300), np.zeros(300)], 1)
    cluster = np.concatenate([rng.uniform(0, 200, (150, 2)), rng.uniform(0, 200, (150, 2)) + 3.0e6])
    same = np.zeros((40, 2))
    pos = torch.from_numpy(np.concatenate([line, cluster, same]).astype(np.float32))
    counts = [300, 300, 40]
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    got = hip().radius_knn(g(pos), g(gptr), 3, 100.0, 8, True).cpu()
    want = REF.radius_knn(pos, gptr, 3, 100.0, 8, True)
    rows_g, rows_w = _rows_as_sets(got, 640), _rows_as_sets(want, 640)
    for i in range(600):                                             # distinct points: exact lists
        assert rows_g[i] == rows_w[i], i
    for i in range(600, 640):                                        # 40 coincident points: any 9 of them, self included
        assert len(rows_g[i]) == 9 and i in rows_g[i] and all(600 <= j < 640 for j in rows_g[i])


def test_radius_graph_front_end_on_device():
    """data.radius_graph dispatches CUDA positions to the HIP kernels and agrees with its own host path per graph."""
    from cgc_net_amd.data import radius_graph
    rng = np.random.RandomState(11)
    pos = torch.from_numpy(rng.uniform(0, 1200.0, size=(900, 2)).astype(np.float32))
    host = radius_graph(pos, 100.0, None, True, 8)
    dev = radius_graph(pos.to(DEV), 100.0, None, True, 8).cpu()
    key = lambda e: sorted(zip(e[0].tolist(), e[1].tolist()))
    assert key(host) == key(dev)
    batch = torch.cat([torch.zeros(500, dtype=torch.int64), torch.ones(400, dtype=torch.int64)])
    both = radius_graph(pos.to(DEV), 100.0, batch.to(DEV), True, 8).cpu()
    a = radius_graph(pos[:500], 100.0, None, True, 8)
    b = radius_graph(pos[500:], 100.0, None, True, 8) + 500
    assert key(both) == key(torch.cat([a, b], 1))


# ------------------------------------------------------------------ F1: loader front-end on the device
def test_device_collate_matches_host_collate_bit_for_bit():
    from cgc_net_amd.data import Batch, Data, SyntheticCellGraphs
    ds = SyntheticCellGraphs(6, 400, 16, base_seed=9)
    items = [ds[i] for i in range(6)]
    mean, std = torch.linspace(-1.0, 1.0, 16), torch.linspace(0.3, 3.0, 16)
    host = Batch.from_data_list([Data(x=(d.x - mean) / std, pos=d.pos, y=d.y, edge_index=d.edge_index) for d in items])
    for rep in range(3):                                             # staging buffers are reused across calls
        dev = Batch.from_data_list(items, device=DEV, mean=mean, std=std)
        assert dev.x.is_cuda and dev.edge_index.is_cuda and dev.batch.is_cuda
        assert torch.equal(dev.x.cpu(), host.x)                      # IEEE division on both sides
        assert torch.equal(dev.pos.cpu(), host.pos) and torch.equal(dev.y.cpu(), host.y)
        assert torch.equal(dev.batch.cpu(), host.batch) and torch.equal(dev.edge_index.cpu(), host.edge_index)
        assert dev._node_counts == host._node_counts
    bare = [Data(x=d.x, pos=d.pos, y=d.y) for d in items]
    built = Batch.from_data_list(bare, device=DEV, knn=(100.0, 8))
    key = lambda e: sorted(zip(e[0].tolist(), e[1].tolist()))
    assert key(built.edge_index.cpu()) == key(host.edge_index)
    assert torch.equal(built.x.cpu(), torch.cat([d.x for d in items]))


def test_model_step_from_device_front_end():
    """The whole front of the path on the device (collate + graph construction) feeds the model: same loss as host-built."""
    from cgc_net_amd.data import Batch, Data, SyntheticCellGraphs
    from cgc_net_amd import network
    ds = SyntheticCellGraphs(4, 300, 16, base_seed=2)
    items = [ds[i] for i in range(4)]
    torch.manual_seed(0)
    model = network.SoftPoolingGcnEncoder(600, 16, 20, 20, True, True, 20, 3, 0.1, [50], concat=True, load_data_sparse=True).to(DEV)
    model.train()
    _, l_host = model(Batch.from_data_list(items).to(DEV))
    _, l_dev = model(Batch.from_data_list([Data(x=d.x, pos=d.pos, y=d.y) for d in items], device=DEV, knn=(100.0, 8)))
    assert abs(l_host.item() - l_dev.item()) <= 1e-6 * max(1.0, abs(l_host.item()))


# ------------------------------------------------------------------ F3: node samplers (farthest-point sampling)
@pytest.mark.parametrize('counts,frac', [([300], 0.5), ([1800, 1500, 2100, 7], 0.5), ([11404, 9000], 0.35), ([16000], 0.5)])
def test_farthest_point_sampling_matches_the_host_loop(counts, frac):
    """csrc/fps.hip against the reference's FarthestSampler loop (common/utils.py:187-197) on coordinate distances."""
    rng = np.random.RandomState(len(counts) + counts[0])
    n, B = sum(counts), len(counts)
    pos = torch.from_numpy(rng.uniform(0.0, 3000.0, size=(n, 2)).astype(np.float32))
    gptr = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32)
    ks = [int(c * frac) for c in counts]
    optr = torch.tensor(np.cumsum([0] + ks), dtype=torch.int32)
    start = torch.tensor([int(rng.randint(c)) for c in counts], dtype=torch.int32)
    want, got = torch.zeros(sum(ks), dtype=torch.int32), torch.zeros(sum(ks), dtype=torch.int32, device=DEV)
    REF.farthest_point_sample(pos, gptr, B, max(counts), start, optr, want)
    hip().farthest_point_sample(g(pos), g(gptr), B, max(counts), g(start), g(optr), got)
    assert torch.equal(got.cpu(), want)                             # the same picks in the same order


def test_fuse_sampler_structure():
    """'fuse' = 70 % farthest-point + 30 % uniform from the rest (dataflow/data.py:210-219): counts, disjointness,
    per-graph membership; the farthest part reproduces the host loop for the same first pick."""
    from cgc_net_amd.data import sample_nodes_batch
    rng = np.random.RandomState(5)
    counts = [900, 1200, 64]
    pos = torch.from_numpy(rng.uniform(0.0, 2000.0, size=(sum(counts), 2)).astype(np.float32))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    idx, ks = sample_nodes_batch(g(pos), counts, 0.5, 'fuse', generator=gen, start=[3, 5, 7])
    assert ks == [450, 600, 32] and idx.numel() == sum(ks) and torch.unique(idx).numel() == idx.numel()
    gptr = np.cumsum([0] + counts)
    idx_c = idx.cpu().numpy()
    for b in range(3):
        mine = idx_c[(idx_c >= gptr[b]) & (idx_c < gptr[b + 1])]
        assert len(mine) == ks[b]
        kf = int(ks[b] * 0.7)
        far = torch.zeros(kf, dtype=torch.int32)
        REF.farthest_point_sample(pos[gptr[b]:gptr[b + 1]], torch.tensor([0, counts[b]], dtype=torch.int32), 1, counts[b],
                                  torch.tensor([[3, 5, 7][b]], dtype=torch.int32), torch.tensor([0, kf], dtype=torch.int32), far)
        assert set((far.numpy() + gptr[b]).tolist()) <= set(mine.tolist())


# ------------------------------------------------------------------ padded row strides (ops._wide) at the kernel level
@pytest.mark.parametrize('width,ld', [(1140, 1152), (300, 320), (180, 192)])
def test_wide_spmm_and_softmax_with_padded_rows(width, ld):
    """cgc_spmm_graphs / cgc_softmax_* on rows whose stride exceeds the width (128-byte-aligned rows): same results as on
    packed rows, and the padding columns are never written."""
    counts = [130, 97, 260, 3]
    s, sg, n = _graph(counts, True, seed=width)
    gptr = g(torch.tensor(np.cumsum([0] + counts), dtype=torch.int32))
    val = torch.zeros(s['cap'])
    REF.edge_renorm(s['rowptr'], s['col'], n, 0.4, val)
    x = rnd(n, width, seed=2)
    want = torch.zeros(n, width)
    REF.spmm(s['rowptr'], s['col'], None, val, None, None, x, want, n, width)
    xb = torch.full((n, ld), 7.0, device=DEV)
    xb[:, :width] = g(x)
    ob = torch.full((n, ld), -3.0, device=DEV)
    hip().spmm(sg['rowptr'], sg['col'], None, g(val), None, None, xb[:, :width], ob[:, :width], n, width, gptr, len(counts),
               max(counts), 1, ld)
    close(ob[:, :width], want, what='padded spmm')
    assert bool((ob[:, width:] == -3.0).all())
    # softmax forward in place + backward with fused column sums
    z = rnd(n, width, seed=4)
    zb = torch.full((n, ld), 9.0, device=DEV)
    zb[:, :width] = g(z)
    hip().softmax_fwd(zb[:, :width], n, width, zb[:, :width], ld)
    sm = torch.softmax(z, 1)
    close(zb[:, :width], sm, what='padded softmax fwd')
    assert bool((zb[:, width:] == 9.0).all())
    dS = rnd(n, width, seed=5)
    db_ = torch.full((n, ld), 1.0, device=DEV)
    db_[:, :width] = g(dS)
    dx = torch.full((n, ld), 5.0, device=DEV)
    cs = torch.empty(width, device=DEV)
    hip().softmax_bwd(zb[:, :width], db_[:, :width], n, width, dx[:, :width], cs, ld)
    want_dx = sm * (dS - (dS * sm).sum(1, keepdim=True))
    close(dx[:, :width], want_dx, what='padded softmax bwd')
    close(cs, want_dx.sum(0), what='padded softmax bwd column sums')
    assert bool((dx[:, width:] == 5.0).all())


@pytest.mark.parametrize('path,n,Kin,F', [('rows', 3000, 0, 20), ('rows', 900, 0, 1140), ('narrow', 3000, 20, 20), ('narrow', 5000, 8, 8),
                                          ('wide', 2500, 20, 1140), ('wide', 700, 16, 114), ('wide', 13000, 20, 1140)])
def test_forward_bn_statistics_survive_small_variance(path, n, Kin, F):
    """BatchNorm's batch variance where the rows are nearly identical (std ~ 1/100 of the mean per column: the coarsened levels,
    whose clusters have near-identical content).  The statistics are a difference of sums: carried in fp32 they lose
    eps * (mean / std)^2 of the variance (1e-3 here) and with it the gradients of the block (5e-4 on the reference-generated
    tiny_shipped fixture before round 4).  All three producers of the statistics -- the row kernel, the fused narrow SAGE
    forward, the fused wide SAGE forward -- must deliver var to 2e-5 and the mean to 1e-6 of a float64 evaluation."""
    k = hip()
    rs = np.random.RandomState(n + F)
    if path == 'rows':
        base = rs.standard_normal((1, F)).astype(np.float32)
        h = torch.from_numpy(base + 0.01 * rs.standard_normal((n, F)).astype(np.float32)).to(DEV)
    else:
        base = rs.standard_normal((1, Kin)).astype(np.float32)
        agg = torch.from_numpy(base + 0.01 * rs.standard_normal((n, Kin)).astype(np.float32)).to(DEV)
        W = torch.from_numpy(rs.standard_normal((Kin, F)).astype(np.float32) * 0.3).to(DEV)
        b = torch.from_numpy(rs.standard_normal(F).astype(np.float32) * 0.1).to(DEV)
        h = agg @ W + b
    count, eps = float(n + 11), 1e-5
    ld = F if path != 'wide' else ((F + 31) // 32) * 32
    hn = torch.empty(n, ld, device=DEV)[:, :F]
    rinv = torch.empty(n, device=DEV)
    rm, rv = torch.zeros(F, device=DEV), torch.ones(F, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    mean, istd = torch.empty(F, device=DEV), torch.empty(F, device=DEV)
    if path == 'rows':
        hn = torch.empty(n, F, device=DEV)
        k.l2norm_act_bn(h, n, F, True, 1, hn, rinv, count, eps, 0.1, rm, rv, nbt, mean, istd)
    else:
        assert k.sage_wide_fwd(agg, Kin, W, b, n, Kin, F, True, 1, hn, rinv, True, count, eps, 0.1, rm, rv, nbt, mean, istd)
    torch.cuda.synchronize()
    o = torch.relu(hn.double())                               # the kernel's own normalised rows, statistics in float64
    m_ref = o.sum(0) / count
    v_ref = (o * o).sum(0) / count - m_ref * m_ref
    var = 1.0 / istd.double() ** 2 - eps
    live = v_ref > 1e-7                                       # (columns that ReLU switches off entirely have no variance to compare)
    assert int(live.sum()) > F // 4
    assert float(((mean.double() - m_ref).abs() / m_ref.abs().clamp_min(1e-3)).max()) < 1e-6
    rel = float(((var - v_ref).abs() / v_ref)[live].max())
    assert rel < 2e-5, rel
