"""References of the edge-weight kernels of csrc/csr.hip (k_edge_renorm, k_csr_invdeg, k_transpose_vals) and the layout kernels of
csrc/exec.hip (k_cat_cols, k_transpose) for tests/test_glue_ref_cpu.py and tests/test_glue_gpu.py.

cgc_edge_renorm, cgc_csr_transpose_vals, cgc_cat_cols and cgc_transpose are compared bit for bit: the first is restated in numpy
float32 (one division, one subtraction and one product per row, each rounded once and none of them contractible into an fma), the
others move or add single floats.  cgc_csr_invdeg sums a row's weights in float32 in slot order: deg - 1 additions and one division,
each within 2^-24 relative on positive terms, so it is held within (deg + 1) * 2^-24 relative to the float64 value (INVDEG_K).

Graphs: row r has degree DEGREES[r % 36] (tests/spmm_ref.py: 0..28, 31, 32, 33, 63, 64, 65, 130) and kind KINDS[r % 5], so every
degree meets every kind once n reaches 180.  ``route`` restates the launches with their constants read from the source text."""
import collections
import ctypes
import functools
import os
import re

import numpy as np
import torch

from rowops_ref import CANARY, Bag, Excess, Place  # noqa: F401
from spmm_ref import DEGREES

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cgc-net_amd', 'csrc')
RENORM_EPS = np.float32(1e-15)
P_RENORM = 0.4
U = 2.0 ** -24
SPARE = 7                                    # slots of val / t_val beyond nnz: they keep the canary
KINDS = ('self_only', 'no_self', 'empty', 'below_one', 'exactly_one')
CSR_N = (255, 256, 257, 1)


# ------------------------------------------------------------------------------------------------ the launches, restated
@functools.lru_cache(maxsize=None)
def source_constants():
    """-> Bag(row_block: threads (= rows) per workgroup of the three CSR kernels; cat_block, cat_cap: k_cat_cols' workgroup size and
    grid cap; tile: k_transpose's tile edge; max_src: the most sources cgc_cat_cols takes)."""
    with open(os.path.join(CSRC, 'csr.hip')) as f:
        csr = f.read()
    with open(os.path.join(CSRC, 'exec.hip')) as f:
        ex = f.read()
    blocks = set()
    for kern in ('k_transpose_vals', 'k_edge_renorm', 'k_csr_invdeg'):
        m = re.search(r'hipLaunchKernelGGL\(%s, dim3\(ceil_div\(n, (\d+)\)\), dim3\((\d+)\)' % kern, csr)
        assert m and m.group(1) == m.group(2), kern
        blocks.add(int(m.group(1)))
    assert len(blocks) == 1
    cat = re.search(r'hipLaunchKernelGGL\(k_cat_cols, dim3\(\(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\)\), dim3\((\d+)\)', ex)
    assert cat and cat.group(1) == cat.group(2) and 'const long long blocks = (total + 255) / 256;' in ex
    tr = re.search(r'hipLaunchKernelGGL\(k_transpose, dim3\(\(unsigned\)ceil_div\(cols, (\d+)\), \(unsigned\)ceil_div\(rows, (\d+)\)\)', ex)
    assert tr and tr.group(1) == tr.group(2) and '__shared__ float t[%s][%d];' % (tr.group(1), int(tr.group(1)) + 1) in ex
    src = re.search(r'if \(nsrc < 1 \|\| nsrc > (\d+)\) return CGC_EINVAL;', ex)
    return Bag(row_block=blocks.pop(), cat_block=int(cat.group(3)), cat_cap=int(cat.group(1)), tile=int(tr.group(1)),
               max_src=int(src.group(1)))


def route_rows(n):
    """-> (workgroups, threads of the last one that own a row) of the one-thread-per-row CSR kernels; (0, 0): no launch."""
    b = source_constants().row_block
    return (0, 0) if n <= 0 else (-(-n // b), n - (-(-n // b) - 1) * b)


def route_cat(rows, total):
    """-> (workgroups, grid-stride passes of the busiest thread) of k_cat_cols; (0, 0): no launch."""
    k = source_constants()
    if rows <= 0 or total <= 0:
        return 0, 0
    blocks = min(-(-rows * total // k.cat_block), k.cat_cap)
    return blocks, -(-rows * total // (blocks * k.cat_block))


def route_transpose(rows, cols):
    """-> (tiles along cols, tiles along rows, whether a tile is cut by an edge)."""
    t = source_constants().tile
    return -(-cols // t), -(-rows // t), bool(rows % t or cols % t)


# ------------------------------------------------------------------------------------------------ CSR inputs
@functools.lru_cache(maxsize=None)
def graph(n):
    """-> Bag(n, nnz, cap, rowptr [n + 1], col [cap], kind [n], deg [n], w [cap] float32 weights for invdeg, t_rowptr, t_perm).
    Kinds: only a self-loop; no self-loop; empty; weights that sum to 0.6 (the clamp at 1 acts); weights that sum to exactly 1
    (1 - (deg - 1) / 1024 and deg - 1 times 1 / 1024: every partial sum is exact).  Rows of the other kinds carry a self-loop and
    weights in (0.5, 1.5).  In a graph of one node only the self-loop exists."""
    rs = np.random.RandomState(n)
    rowptr, col, w, kinds, degs = [0], [], [], [], []
    for r in range(n):
        kind, deg = KINDS[r % len(KINDS)], min(DEGREES[r % len(DEGREES)], max(n - 1, 1))
        if n == 1:
            kind = 'self_only'
        if kind == 'self_only':
            cols = [r]
        elif kind == 'empty' or deg == 0:
            kind, cols = 'empty', []
        else:
            others = rs.choice(n - 1, size=deg if kind == 'no_self' else deg - 1, replace=False)
            cols = sorted([int(c) + (int(c) >= r) for c in others] + ([] if kind == 'no_self' else [r]))
        d = len(cols)
        if kind == 'below_one':
            ww = rs.uniform(0.5, 1.5, d)
            ww = (ww / ww.sum() * 0.6).astype(np.float32)
        elif kind == 'exactly_one':
            ww = np.full(d, 1.0 / 1024, dtype=np.float32)
            ww[0] = 1.0 - (d - 1) / 1024.0
        else:
            ww = rs.uniform(0.5, 1.5, d).astype(np.float32)
        col += cols
        w += ww.tolist()
        rowptr.append(len(col))
        kinds.append(kind), degs.append(d)
    nnz = len(col)
    cap = nnz + SPARE
    colp = np.full(cap, -7, dtype=np.int32)
    colp[:nnz] = col
    wp = np.full(cap, np.nan, dtype=np.float32)
    wp[:nnz] = w
    order = np.argsort(colp[:nnz], kind='stable').astype(np.int32)
    t_perm = np.full(cap, 2 ** 30, dtype=np.int32)            # a read past nnz would index far outside val
    t_perm[:nnz] = order
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(colp[:nnz], minlength=n))]).astype(np.int32)
    return Bag(n=n, nnz=nnz, cap=cap, rowptr=np.asarray(rowptr, dtype=np.int32), col=colp, kind=kinds, deg=np.asarray(degs), w=wp,
               t_rowptr=t_rowptr, t_perm=t_perm)


# ------------------------------------------------------------------------------------------------ CSR references
CSR_MUTANTS = ('renorm_counts_self', 'invdeg_no_clamp', 'invdeg_drops_last', 'tvals_identity')


def edge_renorm(g, p=P_RENORM, mutant=None):
    """The kernel's float32 arithmetic restated: w = (1 / (float(off) + 1e-15f)) * (1 - p), val = p on the diagonal, w elsewhere.
    -> val [cap] float32 with CANARY beyond nnz.  (The 1e-15 is below float32's resolution wherever off >= 1, and where off = 0 no
    off-diagonal weight is stored: it cannot change a bit of val.)"""
    one, p32 = np.float32(1), np.float32(p)
    val = np.full(g.cap, CANARY, dtype=np.float32)
    for r in range(g.n):
        s, e = int(g.rowptr[r]), int(g.rowptr[r + 1])
        off = int(np.count_nonzero(g.col[s:e] != r)) if mutant != 'renorm_counts_self' else e - s
        denom = np.float32(off) + RENORM_EPS
        with np.errstate(divide='ignore'):
            w = np.float32(np.float32(one / denom) * np.float32(one - p32))
        val[s:e] = np.where(g.col[s:e] == r, p32, w)
    return val


def transpose_vals(g, val, mutant=None):
    t = np.full(g.cap, CANARY, dtype=np.float32)
    t[:g.nnz] = val[:g.nnz] if mutant == 'tvals_identity' else val[g.t_perm[:g.nnz]]
    return t


def invdeg(g, w, dtype=np.float64, mutant=None):
    """1 / max(sum of the row's weights, 1) (w None: the degree) -> (out [n], deg [n]); float32: the kernel's order of additions."""
    out = np.empty(g.n, dtype=dtype)
    for r in range(g.n):
        s, e = int(g.rowptr[r]), int(g.rowptr[r + 1])
        if mutant == 'invdeg_drops_last' and e > s:
            e -= 1
        if w is None:
            acc = dtype(e - s)
        else:
            acc = dtype(0)
            for v in w[s:e]:
                acc = dtype(acc + dtype(v))
        if mutant != 'invdeg_no_clamp' or acc == 0:
            acc = max(acc, dtype(1))
        out[r] = dtype(1) / acc
    return out


def excess_invdeg(g, got, want):
    """|got - want| / ((deg + 1) * 2^-24 * want), the largest over the rows; inf for a non-finite value."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != want.shape or not np.isfinite(got).all():
        return float('inf')
    return float(np.max(np.abs(got - want) / ((g.deg + 1) * U * want))) if g.n else 0.0


# ------------------------------------------------------------------------------------------------ layout cases and references
Cat = collections.namedtuple('Cat', 'rows widths pads ldd_pad')
CAT_CASES = (
    Cat(5, (3,), (0,), 0),
    Cat(1, (1,), (2,), 1),
    Cat(7, (1, 4), (3, 0), 2),
    Cat(9, (2, 0, 5), (1, 2, 3), 3),                  # a zero-width source in the middle
    Cat(6, (4, 1, 7, 2), (0, 1, 0, 5), 1),
    Cat(3, (0, 2, 0, 1), (1, 1, 1, 1), 4),            # zero-width sources first and between
    Cat(1100, (300, 1, 0, 699), (4, 0, 1, 1), 8),     # 1.1e6 elements: past 4096 workgroups of 256, the grid-stride second pass
)
Cat.name = property(lambda c: 'r%d-%s' % (c.rows, 'x'.join(str(w) for w in c.widths)))
CAT_MUTANTS = ('cat_zero_width_shift', 'cat_accumulate_ignored', 'cat_second_pass_dropped')
TRANSPOSE_CASES = ((1, 1), (31, 33), (32, 32), (33, 65), (70, 3))


@functools.lru_cache(maxsize=None)
def cat_inputs(case):
    rs = np.random.RandomState([case.rows, len(case.widths), sum(case.widths)])
    srcs = [rs.standard_normal((case.rows, w)).astype(np.float32) for w in case.widths]
    return Bag(srcs=srcs, dst0=rs.standard_normal((case.rows, sum(case.widths))).astype(np.float32))


def cat_cols(case, accumulate, mutant=None):
    """-> dst [rows, total]: the sources side by side, added to dst0 in float32 when accumulate."""
    c = cat_inputs(case)
    srcs = list(c.srcs)
    if mutant == 'cat_zero_width_shift' and 0 in case.widths[:-1]:
        k = case.widths.index(0)                       # the column range of the source after a zero-width one starts one late
        srcs[k + 1] = np.roll(srcs[k + 1], 1, axis=1)
    cat = np.concatenate(srcs, axis=1)
    if mutant == 'cat_second_pass_dropped':
        k = source_constants()
        flat = cat.reshape(-1).copy()
        flat[k.cat_cap * k.cat_block:] = CANARY if not accumulate else 0.0
        cat = flat.reshape(cat.shape)
    if accumulate and mutant != 'cat_accumulate_ignored':
        return (c.dst0 + cat).astype(np.float32)
    return cat


@functools.lru_cache(maxsize=None)
def transpose_input(rows, cols):
    return np.random.RandomState([rows, cols]).standard_normal((rows, cols)).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))


# ------------------------------------------------------------------------------------------------ the direct calls
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_csr(k, P, g, p=P_RENORM, n=None):
    """cgc_edge_renorm into a canary-filled val [cap] (the spare slots beyond nnz are part of what comes back, so that they can be
    compared); cgc_csr_transpose_vals of it; cgc_csr_invdeg over the prescribed weights and without values.  ``n`` overrides the row
    count passed (0: nothing may be written).  -> Bag of numpy arrays (val, t_val, inv_w, inv_deg) and the return codes."""
    n = g.n if n is None else n
    rowptr, col = P.inp(_t(g.rowptr)), P.inp(_t(g.col))
    t_rowptr, t_perm, w = P.inp(_t(g.t_rowptr)), P.inp(_t(g.t_perm)), P.inp(_t(g.w))
    val, t_val, inv_w, inv_deg = P.out(g.cap), P.out(g.cap), P.out(g.n), P.out(g.n)
    s = k._stream()
    rc = [k.lib.cgc_edge_renorm(_ptr(rowptr), _ptr(col), n, p, _ptr(val), s),
          k.lib.cgc_csr_transpose_vals(_ptr(t_rowptr), _ptr(t_perm), _ptr(val), n, _ptr(t_val), s),
          k.lib.cgc_csr_invdeg(_ptr(rowptr), _ptr(w), n, _ptr(inv_w), s),
          k.lib.cgc_csr_invdeg(_ptr(rowptr), None, n, _ptr(inv_deg), s)]
    torch.cuda.synchronize()
    return Bag(rc=rc, val=val.cpu().numpy(), t_val=t_val.cpu().numpy(), inv_w=inv_w.cpu().numpy(), inv_deg=inv_deg.cpu().numpy())


def run_cat(k, P, case, accumulate, nsrc=None):
    """cgc_cat_cols on sources with row stride width + pad into a dst with row stride total + ldd_pad; dst holds dst0 when
    accumulating and the canary otherwise.  nsrc overrides the count passed (the refusals).  -> (rc, dst numpy)"""
    c = cat_inputs(case)
    total = sum(case.widths)
    views = []
    for a, w, pad in zip(c.srcs, case.widths, case.pads):
        views.append(P.inp(_t(a), ld=w + pad) if w else P.inp(torch.zeros(4)))
    dst = P.out(case.rows, total, ld=total + case.ldd_pad)
    if accumulate:
        dst.copy_(_t(c.dst0))
    n = len(views)
    srcs = (ctypes.c_void_p * n)(*[v.data_ptr() for v in views])
    lds = (ctypes.c_int * n)(*[w + pad for w, pad in zip(case.widths, case.pads)])
    widths = (ctypes.c_int * n)(*case.widths)
    rc = k.lib.cgc_cat_cols(_ptr(dst), total + case.ldd_pad, case.rows, n if nsrc is None else nsrc, srcs, lds, widths, int(accumulate),
                            k._stream())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()


def run_transpose(k, P, rows, cols):
    src = P.inp(_t(transpose_input(rows, cols)), ld=cols + 3)
    dst = P.out(cols, rows, ld=rows + 2)
    rc = k.lib.cgc_transpose(_ptr(src), cols + 3, rows, cols, _ptr(dst), rows + 2, k._stream())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()
