"""Float64 reference of the DiffPool regulariser kernels (csrc/diffpool_reg.hip: k_reg_entropy<4> / <1>, k_reg_sumsq, k_reg_trace,
k_reg_finalize behind cgc_diffpool_reg_fwd; cgc_diffpool_reg_bwd_prep, cgc_diffpool_reg_entropy_bwd, cgc_diffpool_reg_adj_bwd) for
tests/test_reg_ref_cpu.py and tests/test_reg_fp64_gpu.py.  The reference is numpy float64 on the float32 inputs the kernels receive;
G and A_out are inputs here, not products under test.

Yardsticks, in units of u = 2^-24 (every excess is an error over its allowance and must be <= 1):

  entropy sum   a lane adds its terms of a row in float32 (VEC * ceil(C / (64 VEC)) of them: one rounding less than that), each term is
                one product and one logf; lanes, rows and workgroups are combined in double (nothing at this scale):
                    |e - ref| <= u * ((adds + 1) * sum s |log(s + eps)|  +  LOGF_GRANTED * sum s (|log(s + eps)| + s / (s + eps)))
                The second sum is the unit the device logf was measured in (below) times s; where it is zero, e is exactly zero.
  a2, g2, tr    products and sums in double: DSUM_K = 64 roundings of 2^-53 (a thread's chain of at most 12 additions, 6 shuffle
                steps, 4 waves, 2 strided partials, 8 shuffle steps, 4 waves again: 36) on a2 + 2 |tr| + g2 =: dT
  link, keep    float32 rounding of the float64 value plus the propagated dT: dT / (2 sqrt(T) numel), dT / (2 sqrt(T));
                T <= 0 (only in the integer-valued finalize cases, where every sum is exact): exactly 0
  ent           float32 rounding of the float64 value plus the entropy allowance / rows
  bwd_prep      bit for bit against ``bwd_prep`` in numpy float32: coef is a double quotient cast to float, 2 c and 4 c are exact,
                every element of dao and Gs is one float32 operation
  entropy_bwd   per element, ds0 + c g with g = -log(s + eps) - s / (s + eps):
                    u * (LOGF_GRANTED |c| (|log| + |ratio|) + |c g| + (|ds0| + |c g|))      (g; the product; the final add)
  adj_bwd       without accumulate one product, bit for bit; with accumulate two roundings (or one, contracted): 2 u (|2 c A| + |gA|)

The device logf cannot be derived.  It is measured on the GPU through cgc_diffpool_reg_entropy_bwd with coef[1] = 1 and ds = 0 (the
product by 1 and the add to 0 are exact), which returns g(s) per element, over SWEEP (s in (0, 1]: 40 decades, the float32
neighbours of 1e-15, of every power of two down to 2^-60 and of 1, and 60000 uniform draws), against float64, in units of
u (|log term| + |ratio term|); twice the measured maximum, rounded up, is granted (the compiler may or may not contract the final
subtraction into the division's last step).

    LOGF_TABLE    measured on an MI355X    granted
    g(s)          3.668 (at s = 1.87e-21)  8

``route`` restates row_vec, grid_for and the grid caps with the constants read from the source text.  The float32 twins restate the
kernels' float32 arithmetic on the CPU (numpy's float32 log in place of the device's) and must pass every judge; ``mutant`` turns
them into one of MUTANTS."""
import collections
import ctypes
import functools
import os
import re

import numpy as np
import torch

from rowops_ref import Bag, Excess, Place  # noqa: F401 (re-exported for the two test files)

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cgc-net_amd', 'csrc', 'diffpool_reg.hip')
U = 2.0 ** -24
EPS = 1e-15
EPS32 = np.float32(1e-15)
DSUM_K = 64
LOGF_MEASURED = 3.668        # the table above
LOGF_GRANTED = 8
MUTANTS = ('eps_missing', 'no_ratio_term', 'diag_wrong_element', 'sumsq_reads_cap', 'vector_tail_dropped', 'sqrt_negative',
           'accumulate_ignored')


# ------------------------------------------------------------------------------------------------ the launches, restated
@functools.lru_cache(maxsize=None)
def source_constants():
    with open(SOURCE) as f:
        text = f.read()
    k = Bag(block=int(re.search(r'#define REG_BLOCK (\d+)', text).group(1)), parts=int(re.search(r'#define REG_PARTS (\d+)', text).group(1)))
    k.ent_bwd_cap = int(re.search(r'const int blocks = grid_for\(\(int64_t\)n \* 64, (\d+)\);', text).group(1))
    k.adj_bwd_cap = int(re.search(r'hipLaunchKernelGGL\(k_reg_adj_bwd, dim3\(grid_for\(m, (\d+)\)\)', text).group(1))
    m = re.search(r'hipLaunchKernelGGL\(k_reg_bwd_prep, dim3\(rows_bc < (\d+) \? rows_bc : (\d+)\)', text)
    assert m.group(1) == m.group(2)
    k.prep_cap = int(m.group(1))
    assert 'inline bool row_vec(const float* a, int C, int ld) { return C % 4 == 0 && ld % 4 == 0 && aligned16(a); }' in text
    assert 'return (int)(b < 1 ? 1 : b > cap ? cap : b);' in text and 'const int64_t b = (work + REG_BLOCK - 1) / REG_BLOCK;' in text
    assert 'rp.n_ent = grid_for((int64_t)(n > 0 ? n : 1) * 64, REG_PARTS);' in text
    assert 'const int64_t a_work = rowptr != nullptr ? (int64_t)REG_PARTS * REG_BLOCK * 4 : A_numel / 4;' in text
    assert '#define REG_EPS 1e-15f' in text
    return k


def grid_for(work, cap):
    b = -(-work // source_constants().block)
    return max(1, min(b, cap))


def route_rows(n, C, ld, aligned, cap=None):
    """The one-wave-per-row kernels (k_reg_entropy: cap REG_PARTS; k_reg_entropy_bwd: cap 4096) -> Bag(vec, blocks, row_passes,
    lane_passes, adds: float32 additions of a lane per row that round)."""
    k = source_constants()
    vec = 4 if C % 4 == 0 and ld % 4 == 0 and aligned else 1
    blocks = grid_for(max(n, 1) * 64, k.parts if cap is None else cap)
    waves = blocks * (k.block // 64)
    lane_passes = -(-C // (64 * vec))
    return Bag(vec=vec, blocks=blocks, row_passes=-(-n // waves), lane_passes=lane_passes, adds=vec * lane_passes - 1)


def route_sumsq(m, aligned, csr=False):
    """k_reg_sumsq -> Bag(blocks, vec_passes: grid-stride passes of the vector loop, tail: elements of the scalar loop)."""
    k = source_constants()
    blocks = grid_for(k.parts * k.block * 4 if csr else m // 4, k.parts)
    m4 = m // 4 if aligned else 0
    return Bag(blocks=blocks, vec_passes=-(-m4 // (blocks * k.block)), tail=m - 4 * m4)


def route_flat(m):
    """k_reg_adj_bwd -> (blocks, passes)."""
    k = source_constants()
    blocks = grid_for(m, k.adj_bwd_cap)
    return blocks, -(-m // (blocks * k.block))


def route_prep(B, C):
    """k_reg_bwd_prep -> (blocks, row passes, column passes)."""
    k = source_constants()
    blocks = min(B * C, k.prep_cap)
    return blocks, -(-B * C // blocks), -(-C // k.block)


# ------------------------------------------------------------------------------------------------ inputs
ROW_KINDS = ('softmax', 'one_hot', 'zero', 'uniform', 'tiny')


def rows_matrix(n, C, seed=0):
    """[n, C] float32, row i of kind ROW_KINDS[i % 5]: a random softmax row; a one-hot row (exactly 1 and exactly 0); an all-zero
    padded row; a uniform 1/C row; a softmax row with entries replaced by 1e-30, 1e-20, 1e-15 and 1e-8."""
    rs = np.random.RandomState([n, C, seed])
    z = rs.standard_normal((n, C)) * 3
    S = np.exp(z - z.max(1, keepdims=True))
    S = (S / S.sum(1, keepdims=True)).astype(np.float32)
    for i in range(n):
        kind = ROW_KINDS[i % 5]
        if kind == 'one_hot':
            S[i] = 0
            S[i, rs.randint(C)] = 1
        elif kind == 'zero':
            S[i] = 0
        elif kind == 'uniform':
            S[i] = np.float32(1) / np.float32(C)
        elif kind == 'tiny':
            for j, v in zip(rs.permutation(C)[:4], (1e-30, 1e-20, 1e-15, 1e-8)):
                S[i, j] = v
    return S


Rows = collections.namedtuple('Rows', 'n C ld off')          # off: floats the base pointer is moved past a 16-byte boundary
ROW_CASES = (
    Rows(37, 4, 4, 0), Rows(5, 260, 264, 0), Rows(2100, 8, 8, 0),                              # k_reg_entropy<4>
    Rows(37, 5, 5, 0), Rows(9, 130, 131, 0), Rows(33, 8, 12, 1), Rows(33, 8, 9, 0), Rows(4, 1, 1, 0), Rows(0, 5, 5, 0),
)
ROW_CASES_BWD = ROW_CASES + (Rows(16400, 4, 4, 0),)
SUMSQ_M = (0, 1, 3, 4, 5, 1023, 1025, 524295)
CSR_NNZ = (5, 1029)
CSR_SPARE = 9
TRACE_BC = ((1, 1), (3, 7), (2, 200))
PREP_BC = ((1, 1), (3, 7), (2, 260), (130, 64))
ADJ_M = (1, 255, 257, 1048581)
# integer-valued (A, G, A_out) of one 1 x 1 graph -> T / (a2 + 2 |tr| + g2)
FINALIZE = collections.OrderedDict([
    ('ratio1', ((3, 4), 2, 0)),                       # T = 29
    ('ratio1e-3', ((44, 8, 1), 1, 999)),              # a2 = 2001, g2 = 1, tr = 999: T = 4 of 4000
    ('ratio1e-6', ((1414, 24, 5, 2), 1, 999999)),     # a2 = 2000001: T = 4 of 4000000
    ('zero', ((2,), 2, 4)),                           # a2 = g2 = tr = 4: T = 0 exactly
    ('negative', ((1,), 1, 4)),                       # T = -6
])
FINALIZE_RATIO = {'ratio1': 1.0, 'ratio1e-3': 1e-3, 'ratio1e-6': 1e-6}


def _rnd(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def _fwd(name, rows, B, G, A_out, A=None, a_off=0, rowptr=None, numel=None, rows_count=None, seed=0):
    S = rows_matrix(rows.n, rows.C, seed)
    return Bag(name=name, rows=rows, S=S, B=B, G=np.asarray(G, dtype=np.float32).reshape(B, rows.C, rows.C),
               A_out=np.asarray(A_out, dtype=np.float32).reshape(B, rows.C, rows.C), A=A, a_off=a_off, rowptr=rowptr,
               numel=float(numel if numel is not None else 7.0), rows_count=float(rows_count if rows_count is not None else 3.0))


@functools.lru_cache(maxsize=None)
def forward_cases():
    """-> OrderedDict name -> Bag(S, rows, B, G, A_out, A, a_off, rowptr, numel, rows_count).  A: dense float32 [m] (rowptr None), or
    the CSR's values [nnz + CSR_SPARE] with NaN beyond nnz (None: all ones) under rowptr [n + 1]."""
    out = collections.OrderedDict()

    def add(c):
        out[c.name] = c
    small = Rows(2, 1, 1, 0)
    for r in ROW_CASES:                                # the entropy kernels: one graph, small G, A_out and A
        C = r.C
        add(_fwd('ent-n%d-C%d-ld%d-off%d' % r, r, 1, 0.1 * _rnd(1, C * C), 0.1 * _rnd(2, C * C), A=_rnd(3, 16), rows_count=1.0))
    for m in SUMSQ_M:                                  # k_reg_sumsq on a dense A: vector path, and the scalar path of a moved base
        for off in (0, 1):
            add(_fwd('sumsq-m%d-off%d' % (m, off), small, 1, [0.0], [0.0], A=_rnd(m, m), a_off=off))          # T = a2
    for nnz in CSR_NNZ:                                # the CSR route: m = rowptr[n], read on the device
        r = Rows(37, 4, 4, 0)
        rowptr = np.minimum(np.arange(r.n + 1) * -(-nnz // r.n), nnz).astype(np.int32)
        val = np.full(nnz + CSR_SPARE, np.nan, dtype=np.float32)
        val[:nnz] = _rnd(nnz, nnz)
        for tag, A, off in (('val', val, 0), ('valmis', val, 1), ('ones', None, 0)):
            add(_fwd('csr-nnz%d-%s' % (nnz, tag), r, 1, 0.1 * _rnd(1, 16), 0.1 * _rnd(2, 16), A=A, a_off=off, rowptr=rowptr))
    for B, C in TRACE_BC:                              # k_reg_trace (and k_reg_sumsq on G [B, C, C])
        add(_fwd('trace-B%d-C%d' % (B, C), Rows(6, C, C, 0), B, _rnd(4, B * C * C), 0.5 * _rnd(5, B * C * C), A=_rnd(6, 64)))
    for name, (A, g, t) in FINALIZE.items():           # k_reg_finalize: integer-valued, every sum exact
        add(_fwd('finalize-' + name, Rows(4, 1, 1, 0), 1, [g], [t], A=np.asarray(A, dtype=np.float32)))
    return out


# ------------------------------------------------------------------------------------------------ the float64 reference
def _ent_parts(S, eps=EPS):
    s = S.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.log(s + eps)
        ratio = s / (s + eps)
    return s, lg, ratio


def entropy(S):
    """-> (sum of -s log(s + eps), sum of s |log(s + eps)|, sum of s (|log(s + eps)| + s / (s + eps)))."""
    s, lg, ratio = _ent_parts(S)
    return float((-s * lg).sum()), float((s * np.abs(lg)).sum()), float((s * (np.abs(lg) + ratio)).sum())


def adjacency_values(c, mutant=None):
    if c.rowptr is None:
        return c.A.astype(np.float64)
    nnz = int(c.rowptr[-1])
    if c.A is None:
        return np.ones(nnz)
    return c.A[:len(c.A) if mutant == 'sumsq_reads_cap' else nnz].astype(np.float64)


def forward(c):
    """-> Bag(e, t_log, t_unit, a2, g2, tr, T, dT, link, ent, keep) in float64."""
    r = Bag()
    r.e, r.t_log, r.t_unit = entropy(c.S)
    a = adjacency_values(c)
    r.a2, r.g2 = float((a * a).sum()), float((c.G.astype(np.float64) ** 2).sum())
    r.tr = float(np.trace(c.A_out.astype(np.float64), axis1=1, axis2=2).sum())
    r.T = r.a2 - 2.0 * r.tr + r.g2
    r.dT = DSUM_K * 2.0 ** -53 * (r.a2 + 2.0 * abs(r.tr) + r.g2)
    root = np.sqrt(r.T) if r.T > 0 else 0.0
    r.link, r.ent, r.keep = root / c.numel, r.e / c.rows_count, root
    return r


def judge_forward(c, ref, link, ent, keep, ex, adds=None):
    """link, ent, keep: the float32 scalars a forward wrote.  Records the excesses under the kernel a case is about."""
    route = route_rows(c.rows.n, c.rows.C, c.rows.ld, c.rows.off == 0)
    adds = route.adds if adds is None else adds
    link, ent, keep = float(link), float(ent), float(keep)
    allow_e = U * ((adds + 1) * ref.t_log + LOGF_GRANTED * ref.t_unit)
    if ref.t_unit == 0:
        ex.add('k_reg_entropy<%d>' % route.vec, 0.0 if ent == 0 else float('inf'))
    else:
        e = abs(ent - ref.ent) / (U * abs(ref.ent) + allow_e / c.rows_count) if np.isfinite(ent) else float('inf')
        ex.add('k_reg_entropy<%d>' % route.vec, e)
    if ref.T <= 0:
        ex.add('k_reg_finalize', 0.0 if link == 0 and keep == 0 else float('inf'))
        return
    slack = ref.dT / (2.0 * ref.keep)
    for name, got, want, div in (('link', link, ref.link, c.numel), ('keep', keep, ref.keep, 1.0)):
        e = abs(got - want) / (U * want + slack / div) if np.isfinite(got) else float('inf')
        ex.add('k_reg_finalize', e)
        ex.add({'sumsq': 'k_reg_sumsq', 'csr': 'k_reg_sumsq', 'trace': 'k_reg_trace'}.get(c.name.split('-')[0], 'k_reg_finalize'), e)


# ------------------------------------------------------------------------------------------------ float32 twins and mutants
def twin_entropy(S, vec, mutant=None):
    """k_reg_entropy<vec>: lane l of a row's wave adds, in float32 and in column order, the terms of columns l * vec + k + 64 vec p;
    the rest in double."""
    n, C = S.shape
    eps = np.float32(0) if mutant == 'eps_missing' else EPS32
    with np.errstate(divide='ignore', invalid='ignore'):
        term = (-S * np.log(S + eps)).astype(np.float32)
    t = np.zeros((n, 64), dtype=np.float32)
    lanes = np.arange(64)
    for p in range(-(-C // (64 * vec))):
        for k in range(vec):
            col = lanes * vec + k + 64 * vec * p
            ok = col < C
            t[:, ok] = t[:, ok] + term[:, col[ok]]
    return float(t.astype(np.float64).sum())


def twin_forward(c, mutant=None):
    """-> (link, ent, keep) as float32, the way the five kernels of cgc_diffpool_reg_fwd form them."""
    route = route_rows(c.rows.n, c.rows.C, c.rows.ld, c.rows.off == 0)
    e = twin_entropy(c.S, route.vec, mutant)
    a = adjacency_values(c, mutant)
    if mutant == 'vector_tail_dropped' and c.rowptr is None and c.a_off == 0:
        a = a[:4 * (len(a) // 4)]
    a2, g2 = float((a * a).sum()), float((c.G.astype(np.float64) ** 2).sum())
    tr = float(np.trace(c.A_out.astype(np.float64), axis1=1, axis2=2).sum())
    T = a2 - 2.0 * tr + g2
    with np.errstate(invalid='ignore'):
        root = np.sqrt(T) if (T > 0 or mutant == 'sqrt_negative') else 0.0
    return np.float32(root / c.numel), np.float32(e / c.rows_count), np.float32(root)


def ent_grad64(S):
    """-> (g = -log(s + eps) - s / (s + eps), |log term| + |ratio term|) in float64."""
    s, lg, ratio = _ent_parts(S)
    return -lg - ratio, np.abs(lg) + ratio


def twin_ent_grad(S, mutant=None):
    eps = np.float32(0) if mutant == 'eps_missing' else EPS32
    with np.errstate(divide='ignore', invalid='ignore'):
        g = -np.log(S + eps)
        if mutant != 'no_ratio_term':
            g = g - S / (S + eps)
    return g.astype(np.float32)


def twin_entropy_bwd(S, ce, ds0, mutant=None):
    return (ds0 + np.float32(ce) * twin_ent_grad(S, mutant)).astype(np.float32)


def judge_entropy_bwd(S, ce, ds0, got):
    """-> the largest excess over the elements of ds[:, :C]."""
    if S.size == 0:
        return 0.0
    g, unit = ent_grad64(S)
    ce = float(np.float32(ce))
    want = ds0.astype(np.float64) + ce * g
    allow = U * (LOGF_GRANTED * abs(ce) * unit + abs(ce * g) + np.abs(ds0.astype(np.float64)) + abs(ce * g))
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float('inf')
    return float((np.abs(got - want) / allow).max())


def bwd_prep(d_reg, keep, numel, rows, d_ao, G, B, C, mutant=None):
    """cgc_diffpool_reg_bwd_prep in numpy float32 -> (coef [2], dao [B, C, C], Gs [B, C, C])."""
    r = float(np.float32(keep))
    cl = np.float32(float(np.float32(d_reg[0])) / (2.0 * numel * r)) if r > 0.0 else np.float32(0)
    coef = np.array([cl, np.float32(float(np.float32(d_reg[1])) / rows)], dtype=np.float32)
    two, four = np.float32(2) * cl, np.float32(4) * cl
    dao = np.zeros((B * C, C), dtype=np.float32) if d_ao is None else d_ao.reshape(B * C, C).astype(np.float32).copy()
    for r_ in range(B * C):
        diag = r_ % C if mutant != 'diag_wrong_element' else (r_ % C + r_ // C) % C      # right in the first graph only
        dao[r_, diag] = dao[r_, diag] - two
    return coef, dao.reshape(B, C, C), (four * G.reshape(B, C, C).astype(np.float32)).astype(np.float32)


def twin_adj_bwd(A, c0, gA0, accumulate, mutant=None):
    v = (np.float32(2) * np.float32(c0)) * A
    return (gA0 + v).astype(np.float32) if accumulate and mutant != 'accumulate_ignored' else v.astype(np.float32)


def judge_adj_bwd(A, c0, gA0, accumulate, got):
    """Bit for bit without accumulate (0 or inf); two roundings of |2 c A| + |gA| with it."""
    v32 = (np.float32(2) * np.float32(c0)) * A
    if not accumulate:
        return 0.0 if np.array_equal(np.asarray(got, dtype=np.float32).view(np.int32), v32.astype(np.float32).view(np.int32)) else float('inf')
    v = 2.0 * float(np.float32(c0)) * A.astype(np.float64)
    want = gA0.astype(np.float64) + v
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float('inf')
    return float((np.abs(got - want) / (2 * U * (np.abs(v) + np.abs(gA0.astype(np.float64))))).max())


@functools.lru_cache(maxsize=None)
def sweep():
    """s in (0, 1] for the logf measurement, [1024, 64] float32."""
    rs = np.random.RandomState(2024)
    v = [np.logspace(-38, 0, 2001), rs.uniform(0, 1, 60000)]
    near = lambda x, k=8: np.float32(x).view(np.int32) + np.arange(-k, k + 1)
    ints = np.concatenate([near(1e-15, 64)] + [near(2.0 ** -j) for j in range(0, 61)])
    f = ints.astype(np.int32).view(np.float32).astype(np.float64)
    s = np.concatenate(v + [f]).astype(np.float32)
    s = s[(s > 0) & (s <= 1)]
    s = np.resize(s, (1024, 64))
    return s


# ------------------------------------------------------------------------------------------------ the direct calls
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def at(dev, a, off=0, ld=None):
    """A device copy of numpy ``a`` whose first element sits ``off`` floats past a 16-byte boundary; 2-D with row stride ld."""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))
    if ld is None or t.dim() != 2:
        buf = torch.zeros(t.numel() + off + 4, dtype=t.dtype, device=dev)
        v = buf[off:off + t.numel()].view(t.shape)
    else:
        buf = torch.zeros(t.shape[0] * ld + off + 4, dtype=t.dtype, device=dev)
        v = buf[off:off + t.shape[0] * ld].view(t.shape[0], ld)[:, :t.shape[1]]
    v.copy_(t)
    return v


def run_forward(k, P, c):
    """cgc_diffpool_reg_fwd -> (link, ent, keep) float32 scalars."""
    dev = P.dev
    S = at(dev, c.S, c.rows.off, c.rows.ld) if c.rows.n else at(dev, np.zeros(4, dtype=np.float32), c.rows.off)
    G, Ao, A, rowptr = at(dev, c.G), at(dev, c.A_out), at(dev, c.A, c.a_off), at(dev, c.rowptr)
    if A is not None and A.numel() == 0:               # an empty tensor has no address: pass one, with A_numel = 0
        A = at(dev, np.zeros(4, dtype=np.float32), c.a_off)
    ws = torch.empty(int(k.lib.cgc_diffpool_reg_ws_floats()), dtype=torch.float32, device=dev)
    link, ent, keep = P.out(1), P.out(1), P.out(1)
    a_numel = 0 if c.rowptr is not None else int(c.A.size)
    rc = k.lib.cgc_diffpool_reg_fwd(_ptr(S), c.rows.n, c.rows.C, c.rows.ld, _ptr(G), _ptr(Ao), c.B, _ptr(A), a_numel, _ptr(rowptr),
                                    c.numel, c.rows_count, _ptr(ws), _ptr(link), _ptr(ent), _ptr(keep), k._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(np.float32(t.cpu().numpy()[0]) for t in (link, ent, keep))


def run_bwd_prep(k, P, d_reg, keep, numel, rows, d_ao, G, B, C):
    dev = P.dev
    dao, Gs, coef = P.out(B * C * C), P.out(B * C * C), P.out(2)
    d_reg, keep = at(dev, np.asarray(d_reg, dtype=np.float32)), at(dev, np.asarray([keep], dtype=np.float32))
    d_ao, G = at(dev, d_ao), at(dev, G)                # named: the operands stay allocated until the kernel has run
    rc = k.lib.cgc_diffpool_reg_bwd_prep(_ptr(d_reg), _ptr(keep), float(numel), float(rows), _ptr(d_ao), _ptr(dao), _ptr(G), _ptr(Gs),
                                         B, C, _ptr(coef), k._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return coef.cpu().numpy(), dao.cpu().numpy().reshape(B, C, C), Gs.cpu().numpy().reshape(B, C, C)


def run_entropy_bwd(k, P, S, rows, ce, ds0, ldd):
    """cgc_diffpool_reg_entropy_bwd with coef = [NaN, ce] (coef[0] is not this kernel's) onto ds0 -> ds [n, C]."""
    dev = P.dev
    n, C = rows.n, rows.C
    Sd = at(dev, S, rows.off, rows.ld) if n else at(dev, np.zeros(4, dtype=np.float32))
    coef = at(dev, np.asarray([np.nan, ce], dtype=np.float32))
    ds = P.out(max(n, 1), C, ld=ldd)
    if n:
        ds.copy_(torch.from_numpy(np.array(ds0)))
    rc = k.lib.cgc_diffpool_reg_entropy_bwd(_ptr(Sd), n, C, rows.ld, _ptr(coef), _ptr(ds), ldd, k._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ds.cpu().numpy()[:n] if n else ds.cpu().numpy()


def run_adj_bwd(k, P, A, c0, gA0, accumulate):
    dev = P.dev
    gA = P.out(A.size)
    if accumulate:
        gA.copy_(torch.from_numpy(np.array(gA0)))
    coef, Ad = at(dev, np.asarray([c0, np.nan], dtype=np.float32)), at(dev, A)
    rc = k.lib.cgc_diffpool_reg_adj_bwd(_ptr(Ad), int(A.size), _ptr(coef), _ptr(gA), int(accumulate), k._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return gA.cpu().numpy()
