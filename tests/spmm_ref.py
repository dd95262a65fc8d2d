"""Float64 reference of the gather kernels (csrc/spmm.hip: k_spmm<4>, k_spmm<1>, k_spmm_wide) for tests/test_spmm_ref_cpu.py and
tests/test_spmm_fp64_gpu.py, written from the contract of cgc_spmm / cgc_spmm_graphs in include/cgc_hip.h:

    out[i,:] = post[i] * sum_{k in row i} w_k * pre[col[k]] * x[col[k],:]      w_k = val[perm[k]] / val[k] / 1

with pre and post optional and perm ignored where val is absent.  Beside ``want`` the reference returns ``terms``, the same sum over
absolute values (times |post[i]|), and ``deg``, the row degrees.

The yardstick is derived, not measured: on exact float32 inputs the kernels round once for w * pre, once per FMA and once for
* post, so per element |got - want| <= (deg[i] + 4) * 2**-24 * terms[i,j] (two units of slack for second-order terms), and got is
exactly zero where terms is.  A non-finite output is an infinite excess.  ``excess`` is the largest ratio of an error to that
allowance; the condition is excess <= 1.

Beside the operator: the graph builder with prescribed degrees, the case list the GPU file runs (the CPU file pins the float32
restatement of oracle/flat_ref.py on every one of them and proves that the inputs discriminate), the call sequence (the same code
drives the restatement on the CPU and the HIP kernels), and ``route``: a restatement of launch_gather that is BOOKKEEPING -- it only
serves to assert that the case list reaches every kernel instance and every branch of the block-id arithmetic, and has to follow
csrc/spmm.hip when the dispatch there changes (tests/test_spmm_ref_cpu.py pins the constants it assumes to the source text)."""
import numpy as np
import torch

import rowops_ref as R
from rowops_ref import Bag, CANARY, Excess, Place  # noqa: F401

U32 = 2.0 ** -24              # unit roundoff of float32
SLACK = 4                     # w * pre, * post and two units for what first-order analysis drops

# ------------------------------------------------------------------------------------------------ launch_gather, restated
GATHER_U, SPMM_PASSES, SPMM_CHUNK, SPMM_RUN, WAVES = 9, 2, 2048, 2, 4
LPR_STEPS = (8, 16, 32)       # pick_lpr: chunks <= 8 -> 8, <= 16 -> 16, <= 32 -> 32, else 64


def _cdiv(a, b):
    return -(-a // b)


def pick_lpr(chunks):
    for s in LPR_STEPS:
        if chunks <= s:
            return s
    return 64


def route(width, ld, aligned, has_gptr, has_val, has_perm, has_pre, n, B, nmax):
    """launch_gather's choice.  aligned: x and out both start on a 16-byte boundary.  -> Bag(kernel, VEC, lpr, n_ctiles, graph_chunks,
    n_chunks, blocks_per_ct, rows_per_block, grid, multi_chunk_tiles; for k_spmm_wide also instance = (VAL, PERM, PRE) and
    order_branch: 'formula' (n_chunks % 8 == 0: the grid is always a multiple of 8) / 'reversal' / None without graph chunks).
    BOOKKEEPING: follows csrc/spmm.hip."""
    vec = width % 4 == 0 and ld % 4 == 0 and aligned
    chunks = width // 4 if vec else width
    lpr = pick_lpr(chunks)
    n_ctiles = _cdiv(chunks, lpr)
    wide = vec and lpr == 64
    rpb = WAVES * SPMM_RUN if wide else WAVES * (64 // lpr) * SPMM_PASSES
    graph = bool(has_gptr) and n_ctiles > 1
    if graph:
        bpc, n_chunks = _cdiv(nmax, rpb), B
    else:
        chunk_rows = _cdiv(SPMM_CHUNK, rpb) * rpb
        bpc, n_chunks = chunk_rows // rpb, _cdiv(n, chunk_rows)
    r = Bag(kernel='k_spmm_wide' if wide else 'k_spmm<4>' if vec else 'k_spmm<1>', VEC=4 if vec else 1, lpr=lpr, n_ctiles=n_ctiles,
            graph_chunks=graph, n_chunks=n_chunks, blocks_per_ct=bpc, rows_per_block=rpb, grid=_cdiv(n_chunks * bpc * n_ctiles, 8) * 8,
            multi_chunk_tiles=(not graph) and n_chunks > 1 and n_ctiles > 1, instance=None, order_branch=None)
    if wide:
        r.instance = (bool(has_val), bool(has_val and has_perm), bool(has_pre))
        r.order_branch = None if not graph else 'formula' if n_chunks % 8 == 0 else 'reversal'
    return r


# ------------------------------------------------------------------------------------------------ the operator in float64
def edge_list(rowptr, col, perm, val, pre, n):
    """-> Bag(rows, cols, w): one entry per edge, w = (val[perm[k]] | val[k] | 1) * (pre[col[k]] | 1) in float64."""
    rp = rowptr.long().cpu()
    deg = rp[1:n + 1] - rp[:n]
    nnz = int(rp[n])
    rows = torch.repeat_interleave(torch.arange(n), deg)
    cols = col[:nnz].long().cpu()
    w = torch.ones(nnz, dtype=torch.float64)
    if val is not None:
        v = val.double().cpu()
        w = v[perm[:nnz].long().cpu()] if perm is not None else v[:nnz]
    if pre is not None:
        w = w * pre.double().cpu()[cols]
    return Bag(rows=rows, cols=cols, w=w)


def aggregate(e, post, x, n, cols=None):
    """-> Bag(want, terms, deg) of the edge list e on the columns [cols[0], cols[1]) of x (all of them when None)."""
    lo, hi = cols or (0, x.shape[1])
    want, terms = torch.zeros(n, hi - lo, dtype=torch.float64), torch.zeros(n, hi - lo, dtype=torch.float64)
    for a in range(lo, hi, 256):                 # a column slab at a time: nnz * width doubles would not be small
        b = min(a + 256, hi)
        t = e.w.unsqueeze(1) * x[:, a:b].double().cpu()[e.cols]
        want[:, a - lo:b - lo].index_add_(0, e.rows, t)
        terms[:, a - lo:b - lo].index_add_(0, e.rows, t.abs())
    if post is not None:
        p = post.double().cpu().unsqueeze(1)
        want, terms = want * p, terms * p.abs()
    return Bag(want=want, terms=terms, deg=torch.bincount(e.rows, minlength=n).double(), cols=(lo, hi))


def spmm(rowptr, col, perm, val, pre, post, x, n, cols=None):
    return aggregate(edge_list(rowptr, col, perm, val, pre, n), post, x, n, cols)


def excess(got, ref):
    """The largest |got - want| / ((deg + 4) * 2**-24 * terms); inf for a non-finite element or a nonzero one where terms is zero."""
    g = got.detach().double().cpu()
    if g.shape[1] != ref.want.shape[1]:
        g = g[:, ref.cols[0]:ref.cols[1]]
    assert g.shape == ref.want.shape, (g.shape, ref.want.shape)
    if g.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(g).all()):
        return float('inf')
    zero = ref.terms == 0
    if bool((g[zero] != 0).any()):
        return float('inf')
    allow = (ref.deg + SLACK).unsqueeze(1) * U32 * ref.terms
    if bool(zero.all()):
        return 0.0
    return float(((g - ref.want).abs()[~zero] / allow[~zero]).max())


# ------------------------------------------------------------------------------------------------ graphs with prescribed degrees
# every wide_tail count 0..8 after 0, 1 and 2 full batches of GATHER_U (0..26), and degree = lpr, lpr + 1 and > 2 lpr for every lpr
DEGREES = tuple(range(0, 29)) + (31, 32, 33, 63, 64, 65, 130)
LOW_DEGREES = (0, 1, 2, 3, 8, 9, 10, 19)


def _signed_distinct(rng, count):
    """count float32 values, pairwise distinct, magnitudes in (0.3, 0.8) and (1.25, 1.75) (away from 0 and 1), signs mixed."""
    t = (rng.permutation(count) + 0.5) / max(count, 1)
    m = np.where(t < 0.5, 0.3 + t, 0.75 + t)
    out = (m * np.where(rng.rand(count) < 0.5, -1.0, 1.0)).astype(np.float32)
    assert len(np.unique(np.abs(out))) == count
    return torch.from_numpy(out)


def build_graph(counts, phase, degrees=DEGREES):
    """A block-diagonal batch: row i has degree degrees[(i + phase) % len]; its columns are drawn (with repetition) inside its own
    graph, never from that graph's one ``unref`` node (graphs of two nodes and more), whose row of x will be NaN.  val has 7 slots more
    than edges and perm is a random injection into them.  -> Bag(n, B, nmax, counts, gptr, rowptr, col, perm, val, pre, post, unref)"""
    rng = np.random.RandomState(1000 + 31 * phase + len(counts))
    n = int(sum(counts))
    gp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    deg = np.array([degrees[(i + phase) % len(degrees)] for i in range(n)], dtype=np.int64)
    cols, unref = [], []
    for g, size in enumerate(counts):
        lo = int(gp[g])
        pool = np.arange(lo, lo + size)
        if size >= 2:
            u = lo + (phase + g) % size
            unref.append(u)
            pool = pool[pool != u]
        for i in range(lo, lo + size):
            cols.append(rng.choice(pool, size=deg[i], replace=True))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    nnz = len(col)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    perm = rng.permutation(nnz + 7)[:nnz].astype(np.int32)
    assert nnz < 2 or bool((perm != np.arange(nnz)).any())
    t = torch.from_numpy
    return Bag(n=n, B=len(counts), nmax=int(max(counts)), counts=tuple(counts), gptr=t(gp.astype(np.int32)), rowptr=t(rowptr), col=t(col),
               perm=t(perm), val=_signed_distinct(rng, nnz + 7), pre=_signed_distinct(rng, n), post=_signed_distinct(rng, n),
               unref=unref, deg=deg)


# ------------------------------------------------------------------------------------------------ case list
# B = 8: an empty graph, a one-node graph, the largest graph not first, 64 = a multiple of every rows-per-block (8, 16, 32, 64), 65 = one more
BATCHES = {
    'B8': (37, 0, 1, 130, 64, 9, 300, 65),
    'B16': (8, 9, 17, 5, 0, 1, 33, 12, 16, 24, 3, 40, 7, 11, 2, 20),
    'B5': (20, 0, 65, 8, 33),
    'n2100': (2100,),
}
VEC_WIDTHS = (4, 32, 36, 64, 68, 128)
WIDE_WIDTHS = (132, 256, 260, 516, 1140)
SCALAR_WIDTHS = (1, 3, 7, 13, 18, 33, 63, 65, 129, 257)
# (val, perm, pre, post): the two production combinations -- the forward aggregation and its transpose in the backward
FWD, BWD = (True, False, False, True), (True, True, True, False)
# every weight source x pre x post, plus perm given without val (which must be ignored)
ALL_COMBOS = [(v, p, q, s) for (v, p) in ((False, False), (True, False), (True, True), (False, True)) for q in (False, True)
              for s in (False, True)]
ALL_COMBOS = [c for c in ALL_COMBOS if c[:2] != (False, True) or not c[3]]      # perm without val: with and without pre
ALL_COMBO_WIDTHS = (36, 13, 260)


def combo_name(c):
    return '+'.join(name for name, on in zip(('val', 'perm', 'pre', 'post'), c) if on) or 'plain'


def case(width, combo, batch='B8', pad=0, mis=(), flat=True, graphs=True):
    """A case: rows of x and out have the stride width + pad (the padding columns of x hold NaN, those of out the canary; the flat
    entry has no stride argument and runs at pad = 0 only); the operands named in `mis` ('x', 'out') sit one float past a 16-byte
    boundary."""
    name = 'w%d-%s-%s' % (width, batch, combo_name(combo))
    if pad:
        name += '-ld%d' % (width + pad)
    name += ''.join('-%smis' % m for m in mis)
    return Bag(name=name, width=width, ld=width + pad, combo=tuple(combo), batch=batch, mis=tuple(mis), flat=flat and pad == 0, graphs=graphs,
               phase=width + 5 * ALL_COMBOS.index(tuple(combo)), degrees=LOW_DEGREES if batch == 'n2100' else DEGREES)


def _cases():
    out = []
    every = VEC_WIDTHS + WIDE_WIDTHS + SCALAR_WIDTHS
    for w in every:
        out += [case(w, FWD), case(w, BWD)]
    for i, w in enumerate(every):                            # padded rows that keep the width's route
        out.append(case(w, (BWD, FWD)[i % 2], pad=4))
    for w in (260, 300):                                     # ld % 4 != 0: the scalar kernel with several tiles and gptr
        out += [case(w, FWD, pad=1), case(w, BWD, pad=1)]
    for w in (4, 64, 260):                                   # multiples of 4 sent down the scalar kernel
        out += [case(w, FWD, mis=('x', 'out')), case(w, BWD, mis=('x', 'out'))]
    out += [case(64, FWD, mis=('x',)), case(260, BWD, mis=('out',))]
    for w in ALL_COMBO_WIDTHS:
        out += [case(w, c) for c in ALL_COMBOS if c not in (FWD, BWD)]
    for batch in ('B16', 'B5'):                              # order formulas of k_spmm_wide: n_chunks % 8 == 0 and not
        out += [case(w, BWD, batch) for w in WIDE_WIDTHS] + [case(260, FWD, batch)]
    for w in (65, 260):                                      # rows >= 2048 live in chunk 1, with more than one column tile
        out += [case(w, FWD, 'n2100'), case(w, BWD, 'n2100')]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
BITS_CASE = case(260, BWD)        # the case of the bit-equality test across entry points and visiting orders


def case_route(c, entry):
    g = graph_of(c)
    v, p, q, _ = c.combo
    return route(c.width, c.ld, not c.mis, entry == 'graphs', v, p, q, g.n, g.B, g.nmax)


def launches(c):
    """[Bag(entry, visit, gorder)]: the flat entry (pad = 0), the graph entry, and on k_spmm_wide also visit 1, 2 and a gorder."""
    out = [Bag(entry='flat', visit=0, gorder=False, tag='flat')] if c.flat else []
    if c.graphs:
        out.append(Bag(entry='graphs', visit=0, gorder=False, tag='graphs'))
        if case_route(c, 'graphs').kernel == 'k_spmm_wide':
            out += [Bag(entry='graphs', visit=v, gorder=False, tag='visit%d' % v) for v in (1, 2)]
            out.append(Bag(entry='graphs', visit=0, gorder=True, tag='gorder'))
    return out


_GRAPHS, _REFS = {}, {}


def graph_of(c):
    key = (c.batch, c.phase)
    if key not in _GRAPHS:
        _GRAPHS[key] = build_graph(BATCHES[c.batch], c.phase, c.degrees)
    return _GRAPHS[key]


def inputs(c):
    """-> Bag(g, x [n, ld] with NaN in the padding columns and in the unreferenced nodes' rows, perm, val, pre, post or None)."""
    g = graph_of(c)
    x = torch.full((g.n, c.ld), float('nan'))
    x[:, :c.width] = R._rnd(7000 + c.width + len(g.counts), g.n, c.width)
    for u in g.unref:
        x[u] = float('nan')
    v, p, q, s = c.combo
    return Bag(g=g, x=x, val=g.val if v else None, perm=g.perm if p else None, pre=g.pre if q else None, post=g.post if s else None)


def reference_of(c):
    """The float64 reference of a case, computed once and shared by its placements and by the tests of a module."""
    key = (c.batch, c.phase, c.combo, c.width)
    if key not in _REFS:
        i = inputs(c)
        _REFS[key] = spmm(i.g.rowptr, i.g.col, i.perm, i.val, i.pre, i.post, i.x[:, :c.width], i.g.n)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ placement and call sequence
class Places(object):
    """An aligned and a misaligned rowops_ref.Place; the operands named in `mis` go to the second."""

    def __init__(self, dev, mis=()):
        self.dev, self.a, self.m, self.mis = dev, Place(dev), Place(dev, 'misaligned'), frozenset(mis)

    def of(self, name):
        return self.m if name in self.mis else self.a

    def check(self):
        self.a.check(), self.m.check()


def run(Kn, P, c, i, L):
    """One launch L of case c on kernels Kn.  -> the output view [n, width] inside its canary-filled buffer."""
    g = i.g
    A = P.a
    x = P.of('x').inp(i.x)[:, :c.width]
    out = P.of('out').out(g.n, c.width, c.ld)
    args = (A.inp(g.rowptr), A.inp(g.col), A.inp(i.perm), A.inp(i.val), A.inp(i.pre), A.inp(i.post), x, out, g.n, c.width)
    if L.entry == 'flat':
        Kn.spmm(*args)
    else:
        gorder = None
        if L.gorder:
            gorder = A.inp(torch.from_numpy(np.random.RandomState(g.B).permutation(g.B).astype(np.int32)))
        Kn.spmm(*args, gptr=A.inp(g.gptr), num_graphs=g.B, nmax=g.nmax, visit=L.visit, ld=c.ld, gorder=gorder)
    return out


def check_case(Kn, c, launch):
    """Every launch of a case: ``launch(run)`` calls run(Places) -> output (the GPU file launches twice and asserts containment and
    identical bits).  -> (Excess keyed by '<kernel> <tag>', {tag: output})"""
    i, ref = inputs(c), reference_of(c)
    ex, outs = Excess(), {}
    for L in launches(c):
        o = launch(lambda P: run(Kn, P, c, i, L))
        ex.add('%s/%s' % (case_route(c, L.entry).kernel, L.tag), excess(o, ref))
        outs[L.tag] = o
    return ex, outs


# ------------------------------------------------------------------------------------------------ mutations (the CPU file)
def mutations(c):
    """{name: (got, ref)}: a wrong result of the kind a subtly broken kernel would produce, and the reference to judge it against
    (the first columns of the case, except for the rotation).  A mutation whose operand the case does not have is absent."""
    i, g = inputs(c), graph_of(c)
    full = reference_of(c)
    cols = (0, min(c.width, 8))
    x = i.x[:, :c.width]
    ref = full if cols[1] == c.width else spmm(g.rowptr, g.col, i.perm, i.val, i.pre, i.post, x, g.n, cols)
    e = edge_list(g.rowptr, g.col, i.perm, i.val, i.pre, g.n)
    row = int(np.nonzero(g.deg >= 2)[0][c.phase % 7])                 # a row with edges
    last = int(g.rowptr[row + 1]) - 1
    keep = torch.ones(len(e.w), dtype=torch.bool)
    keep[last] = False
    agg = lambda ee, post=i.post: aggregate(ee, post, x, g.n, cols).want
    out = {'drop the last edge of a row': (agg(Bag(rows=e.rows[keep], cols=e.cols[keep], w=e.w[keep])), ref)}
    twice = torch.cat([torch.arange(len(e.w)), torch.tensor([last - 1])])
    out['duplicate an edge'] = (agg(Bag(rows=e.rows[twice], cols=e.cols[twice], w=e.w[twice])), ref)
    if i.val is not None and i.perm is not None:
        out['val[k] for val[perm[k]]'] = (agg(edge_list(g.rowptr, g.col, None, i.val, i.pre, g.n)), ref)
    if i.pre is not None:
        bare = edge_list(g.rowptr, g.col, i.perm, i.val, None, g.n)
        out['pre by row'] = (agg(Bag(rows=e.rows, cols=e.cols, w=bare.w * i.pre.double()[e.rows])), ref)
    if i.post is not None:
        out['post omitted'] = (agg(e, None), ref)
    vec = case_route(c, 'graphs').VEC
    if c.width > vec:
        got = full.want.clone()
        got[row] = torch.roll(got[row], vec)
        out['column tile shifted by a lane'] = (got, full)
    return out
