"""Float64 reference of the exact fp32 GEMM (csrc/gemm.hip, csrc/gemm_common.hpp: k_gemm_f32<FAST>, k_gemm_f32<!FAST>, k_gemm_f32_shortk,
k_gemm_fixup, k_reduce_batch_sum, k_reduce_many_parts) for tests/test_gemm_ref_cpu.py and tests/test_gemm_fp64_gpu.py, written from the
contract of cgc_gemm_f32 / cgc_reduce_batch_sum / cgc_reduce_batched in include/cgc_hip.h.  Per output element, in float64:

    want  = alpha * (sum over the main pair and the extra K segments of op(A) op(B)) + bias + beta * C0
    terms = |alpha| * sum |a| |b| + |bias| + |beta| |C0|

The yardstick is derived, not measured: |got - want| <= (Ktot + 16) * 2**-24 * terms, Ktot being that element's reduction length, the
extra segments included (ragged 2: the graph's own K; ragged 3: the chunk's K).  It is the standard bound of a sum of Ktot products
with one rounding per operation in any order (the MFMA FMA chain rounds once per term); the 16 covers the alpha multiply, the bias
add, the beta fma, up to 11 slab additions of the tail split and the second-order remainder.  Where terms is zero the result must be
exactly zero; nothing may be non-finite.  ``excess`` is the largest ratio of an error to the allowance; the condition is excess <= 1.

Two input families, every case on both.  'ints': operands in {-3..3}, bias and C0 in {-8..8}, alpha in {1, 0.5, -2}, beta in
{0, 1, -2}: every partial sum is an integer (or half of one) below 2**24, so the result must EQUAL the reference whatever the
summation order -- any dropped, doubled, misplaced or stale element shows, however small.  'reals': magnitudes uniform in [1, 1.25),
random signs, judged by the allowance: a single missing summand exceeds its element's allowance (asserted per case, ``magnitudes_ok``).
For 'reals' there is also the recorded bar of the GPU file: the rms of err / terms against that of a sequential float32 chain on the
same inputs (``chain_rms``).

Buffers (``Places``): operands sit in NaN-filled allocations -- row padding, the gap between batch items and the floats in front of
the base are NaN; C sits in a canary-filled allocation with padding columns, gaps and two spare rows before and after; ``check()``
asserts that every byte outside the logical elements of C is what it was.  A C that beta == 0 must not read starts as NaN.

BOOKKEEPING: ``dispatch`` restates gemm_dispatch (the forcing of cgc_gemm_tuning included), gemm_all_fast, launch_cfg and the TileMap
quantities T, L, S for resident = 512; ``fetch_choices`` the loader sub-choices of the guarded kernel's fetch lambda.  They only serve
to assert that the case list reaches every kernel instance and branch, and have to follow csrc/gemm.hip when the dispatch there
changes (tests/test_gemm_ref_cpu.py pins the constants they assume to the source text).  Every case carries ``route``: the kernel
instance it is expected to reach, its tile shape, its TileMap mode and, where the tail split applies, L and S.

Where to find what (case names; c<cfg> is the value given to cgc_gemm_tuning, 0 = automatic):
    A-*   every instance: 6 tile shapes x {NN, NT, TN} x {FAST (fit, ldcodd, misC), guarded (odd, misA, misB), short-K}; M = BM + 37,
          N = BN + 21; K = 180 / 181 / 183 (pipelined), 41 / 1 (short-K); tail split off, so the kernel's own epilogue runs (TN = 1
          and TN = 2 instances; scalar over the whole tile at ldcodd / misC); '-split': the same through k_gemm_fixup's <1,1> epilogue
    B-*   K % 32 in {0, 1, 7, 8, 9, 24, 25, 31} at K < 32 and at 64 + remainder (nkb at the edges of the 8-wide k groups)
    C-*   tail split: S = 2, 4, 5, 8, 9, 12 on one 128 x 128 tile (the fix-up's remainder loop alone, one pass of four, four + three, two
          passes, two passes + three); S = 5 on the five smaller tile shapes; a piece made of extra segments only (C-xpiece); T > 512 with
          whole tiles and a tail (C-T528: 16 tail tiles; C-T525: T & 7 = 5, tail_slot's second branch); ragged M compact list and
          ragged K serpentine dealing with a tail (C-raggedM, C-raggedK)
    D-*   the three TileMap modes without a tail: ragged 1 NN / NT and ragged 2, 5, 8, 64, 65 and 72 graphs (65, 72: the plain cut with
          empty tiles; 8, 64: rank ties of equal K)
    E-*   ragged = 3 on the automatic route and on cfg 11, and cgc_reduce_batched over its parts
    F-*   extra K segments: 1 and 2, fitting (FAST) and on an odd stride (guarded), flat NT / NN / TN and ragged-M NT, a first segment of
          xK = 0 (compaction), and a forced short-K route with a segment (takes the pipelined kernel of the forced tile shape)
    G-*   K = 0, 1 x 1 x 1, N = 0 / batch = 0 / M = 0 (return 0, write nothing) and every CGC_EINVAL condition (raise, write nothing)
    H     ``h_cases``: one logical product on every instance, equal values (the GPU file's test of its own)
    I     ``REDUCE_PARTS`` x ``REDUCE_NUMEL`` x outer x beta: the reduce kernels (the GPU file's test of its own)
Out of scope: the >= 4 GiB operand limits of gemm_all_fast need operands too large for a quick test."""
import collections
import zlib

import numpy as np
import torch

from rowops_ref import Bag, CANARY, Excess  # noqa: F401

U32 = 2.0 ** -24              # unit roundoff of float32
SLACK = 16
RMS_FACTOR, RMS_FLOOR = 2.0, 2.0 ** -30

# ------------------------------------------------------------------------------------------------ constants of csrc/gemm.hip
BK, RESIDENT, SHORTK_MAX, FILL_MIN, MIN_KT, S_CAP, SPLIT_TILES_MAX = 32, 512, 160, 448, 3, 12, 384
TILES = {1: (2, 2, 2, 2), 2: (4, 1, 1, 2), 3: (1, 4, 2, 1), 4: (2, 2, 1, 1), 5: (4, 1, 1, 1), 6: (1, 4, 1, 1)}     # WGM, WGN, TM, TN
LAYOUTS = {'NN': (False, False), 'NT': (False, True), 'TN': (True, False)}
EPI = ((1.0, 0.0, False), (0.5, 1.0, True), (-2.0, -2.0, False), (1.0, 0.0, True))      # alpha, beta, bias


def _cdiv(a, b):
    return -(-a // b)


def up4(v):
    return (v + 3) & ~3


def tile_dims(t):
    wgm, wgn, tm, tn = TILES[t]
    return wgm * tm * 32, wgn * tn * 32


def lay_name(tA, tB):
    return 'TT' if tA and tB else 'TN' if tA else 'NT' if tB else 'NN'


# ------------------------------------------------------------------------------------------------ cases
def case(name, lay, M, N, K, batch=1, ragged=0, counts=None, chunk=0, outer=1, extras=(), xodd=(), ldA='fit', ldB='fit', ldC='fit',
         mis=(), ep=0, cfg=0, split=True, over=None, expect='ok', seed=None):
    """M, N, K: the logical extents (ragged 1: counts are the graphs' M; ragged 2: the graphs' K; ragged 3: K rows per outer item cut
    into chunks).  extras: xK per extra segment; xodd: the segments on an odd row stride.  ldA / ldB / ldC: 'fit' = up4(width) + 4,
    'odd' = width + 1 (+ 2 where that is a multiple of 4), 'tight' = width.  mis: operands whose base sits one float past a 16-byte
    boundary.  over: call arguments replaced in the launch (the invalid calls of G).  seed: names the inputs (cases with one seed and one
    geometry share their logical operands: H)."""
    tA, tB = LAYOUTS[lay]
    if ragged in (1, 2):
        batch = len(counts)
    if ragged == 3:
        parts = _cdiv(K, chunk)
        batch = outer * parts
        counts = [min(chunk, K - p * chunk) for _ in range(outer) for p in range(parts)]
    alpha, beta, bias = EPI[ep % 4]
    c = Bag(name=name, lay=lay, tA=tA, tB=tB, M=M, N=N, K=K, batch=batch, ragged=ragged, counts=tuple(counts or ()), chunk=chunk,
            outer=outer, extras=tuple(extras), xodd=tuple(xodd), ldA=ldA, ldB=ldB, ldC=ldC, mis=tuple(mis), alpha=alpha, beta=beta,
            bias=bias, cfg=cfg, split=split, over=dict(over or {}), expect=expect, seed=seed or name)
    c.route = dispatch(c)
    return c


def items(c):
    """[(m, k)] per batch item."""
    if c.ragged == 1:
        return [(n, c.K) for n in c.counts]
    if c.ragged >= 2:
        return [(c.M, n) for n in c.counts]
    return [(c.M, c.K)] * c.batch


def ktot(c, k):
    return k + sum(c.extras)


def _ld(width, kind):
    if kind == 'fit':
        return up4(width) + 4
    if kind == 'tight':
        return max(width, 1)
    return width + 1 if (width + 1) % 4 else width + 2


def _stride(rows, ld, kind):
    return rows * ld + (0 if kind == 'tight' else 8 if ld % 4 == 0 else 3)


def placement(c):
    """Row strides, batch strides (0 for an operand whose items are consecutive row blocks) and base alignment of every operand."""
    it = items(c)
    m_rows = max([m for m, _ in it] or [0])
    k_rows = max([k for _, k in it] or [0])
    p = Bag()
    catA, catB, catC = c.ragged >= 1, c.ragged >= 2, c.ragged == 1
    p.lda = _ld(c.M if c.tA else c.K, c.ldA)
    p.ldb = _ld(c.K if c.tB else c.N, c.ldB)
    p.ldc = _ld(c.N, c.ldC)
    p.sA = 0 if catA else _stride(k_rows if c.tA else m_rows, p.lda, c.ldA)
    p.sB = 0 if catB else _stride(c.N if c.tB else k_rows, p.ldb, c.ldB)
    p.sC = 0 if catC else _stride(m_rows, p.ldc, c.ldC)
    p.alA, p.alB, p.alC = 'A' not in c.mis, 'B' not in c.mis, 'C' not in c.mis
    p.xlda, p.xldb, p.xsA, p.xsB = [], [], [], []
    for s, xk in enumerate(c.extras):
        kind = 'odd' if s in c.xodd else 'fit'
        p.xlda.append(_ld(c.M if c.tA else xk, kind))
        p.xldb.append(_ld(xk if c.tB else c.N, kind))
        p.xsA.append(0 if c.ragged == 1 else _stride(xk if c.tA else m_rows, p.xlda[-1], kind))
        p.xsB.append(_stride(c.N if c.tB else xk, p.xldb[-1], kind))
    return p


def call_args(c):
    """The arguments of the launch, ``over`` applied: Bag(tA, tB, M, N, K, batch, ragged, max_ragged, nx, xK, mode)."""
    a = Bag(tA=c.tA, tB=c.tB, M=0 if c.ragged == 1 else c.M, N=c.N, K=0 if c.ragged == 2 else c.K, batch=c.batch, ragged=c.ragged,
            max_ragged=c.chunk if c.ragged == 3 else max(c.counts or (0,)), xK=list(c.extras), mode=0, fake_extras=0)
    for k, v in c.over.items():
        setattr(a, k, v)
    if a.fake_extras:
        a.xK = [8] * a.fake_extras
    a.nx = len(a.xK)
    return a


# ------------------------------------------------------------------------------------------------ gemm_dispatch, restated
def all_fast(c, a=None):
    """gemm_all_fast: every segment fit for the unguarded 16-byte loaders.  (The 4 GiB limits are out of reach of these cases.)"""
    a, p = a or call_args(c), placement(c)

    def seg(alA, alB, lda, ldb, sA, sB, K):
        if lda % 4 or ldb % 4 or not alA or not alB:
            return False
        if a.batch > 1 and (sA % 4 or sB % 4):
            return False
        if (lda < up4(a.M)) if a.tA else (lda < up4(K)):
            return False
        if (ldb < up4(K)) if a.tB else (ldb < up4(a.N)):
            return False
        return True
    if not seg(p.alA, p.alB, p.lda, p.ldb, p.sA, p.sB, 0 if a.ragged >= 2 else a.K):
        return False
    return all(seg(True, True, p.xlda[s], p.xldb[s], p.xsA[s], p.xsB[s], xk) for s, xk in enumerate(c.extras) if xk > 0)


def tile_map(c, a, BM, BN, shortk, split):
    """TileMap::init and GemmPlan for resident = 512: -> Bag(mode, T, L, S, Tdp, slot_branches, launched)."""
    tiles_n = _cdiv(a.N, BN)
    m_extent = a.max_ragged if a.ragged == 1 else a.M
    k_extent = a.max_ragged if a.ragged >= 2 else a.K
    per_batch = _cdiv(m_extent, BM) * tiles_n
    launched = per_batch * a.batch
    kt = _cdiv(k_extent, BK) + sum(_cdiv(x, BK) for x in a.xK if x > 0)
    mode, T = 0, launched
    if a.ragged == 1 and a.batch <= 64:
        mode, T = 1, sum(_cdiv(n, BM) for n in c.counts) * tiles_n
    elif a.ragged == 2 and a.batch <= 64 and a.batch % 8 == 0:
        mode = 2
    r = Bag(mode=mode, T=T, L=0, S=1, Tdp=T, slot_branches=set(), launched=launched, kt=kt, per_batch=per_batch)
    big = (BM, BN) == (128, 128)
    s_max = min(kt // MIN_KT, S_CAP)
    if not shortk and split and (big or launched <= SPLIT_TILES_MAX) and s_max >= 2 and T > 0:
        l = T if T < RESIDENT else T % RESIDENT
        if l > 0:
            s = min((RESIDENT + l // 2) // l, s_max)
            if s >= 2:
                r.L, r.S, r.Tdp = l, s, T - l
                common = ((T >> 3) - (r.Tdp >> 3)) * 8
                r.slot_branches = ({1} if min(l, common) > 0 else set()) | ({2} if l > common else set())
    return r


def dispatch(c):
    """-> Bag(status 'einval' / 'noop' / 'launch'; for a launch: tile (1..6), BM, BN, kernel 'fast' / 'guarded' / 'shortk', lay, and the
    tile_map quantities mode, T, L, S, slot_branches).  BOOKKEEPING: follows gemm_dispatch, launch_cfg and cgc_gemm_f32."""
    a = call_args(c)
    ein, noop = Bag(status='einval'), Bag(status='noop')
    if a.nx > 2 or a.mode not in (0, 1, 2):
        return ein
    nx = sum(1 for x in a.xK if x > 0)
    if a.batch <= 0 or a.N <= 0:
        return noop
    if a.ragged == 1 and a.tA:
        return ein
    if a.ragged == 2 and (not a.tA or a.tB or nx > 0):
        return ein
    if a.ragged == 3 and (not a.tA or a.tB or nx > 0 or a.max_ragged <= 0 or a.K <= 0 or a.batch % _cdiv(a.K, a.max_ragged) != 0):
        return ein
    if a.ragged < 0 or a.ragged > 3:
        return ein
    m_extent = a.max_ragged if a.ragged == 1 else a.M
    if m_extent <= 0:
        return noop
    k_extent = a.max_ragged if a.ragged >= 2 else a.K
    sk = k_extent <= SHORTK_MAX and nx == 0
    fill = _cdiv(m_extent, 128) * a.batch
    force = c.cfg
    if force > 0 and 1 <= force % 10 <= 6:
        tile = force % 10
        sk = (nx == 0) if force >= 20 else False if force >= 10 else sk
    elif a.N <= 32:
        tile = 5
    elif a.N <= 64:
        tile = 4 if m_extent > 64 and fill < FILL_MIN else 2
    elif m_extent <= 32:
        tile = 6
    elif m_extent <= 64:
        tile = 3
    elif fill * _cdiv(a.N, 128) < FILL_MIN:
        if a.N <= 128:
            tile = 5 if k_extent > 256 and m_extent > 128 else 4
        elif a.tA:
            tile = 1 if not sk and c.split and k_extent >= 24 * BK else 2
        else:
            tile = 3
    else:
        tile = 1
    if a.tA and a.tB:
        return ein
    BM, BN = tile_dims(tile)
    r = tile_map(c, a, BM, BN, sk, c.split)
    r.status, r.tile, r.BM, r.BN, r.lay = 'launch', tile, BM, BN, lay_name(a.tA, a.tB)
    r.kernel = 'shortk' if sk else 'fast' if all_fast(c, a) else 'guarded'
    r.instance = (tile, r.kernel, r.lay)
    return r


def fetch_choices(c):
    """The loader sub-choices the guarded kernel's (and the short-K kernel's) fetch lambda takes on this case:
    {(operand 'A' / 'B', 'main' / 'extra', 'load_fast' / 'load_fast_masked' / 'load')}.  BOOKKEEPING: follows k_gemm_f32."""
    r, p, out = c.route, placement(c), set()
    if r.status != 'launch' or r.kernel == 'fast':
        return out
    vecA, vecB = p.lda % 4 == 0 and p.alA, p.ldb % 4 == 0 and p.alB
    for m, k in items(c):
        if m <= 0:
            continue
        fastA = vecA and (p.lda >= up4(m) if c.tA else True)
        fastB = vecB and c.N >= 1 and (True if c.tB else p.ldb >= up4(c.N))
        k4A = k >= 1 and (True if c.tA else p.lda >= up4(k))
        k4B = k >= 1 and (p.ldb >= up4(k) if c.tB else True)
        for kt in range(_cdiv(k, BK)):
            full = kt < k // BK
            out.add(('A', 'main', 'load_fast' if fastA and full else 'load_fast_masked' if fastA and k4A else 'load'))
            out.add(('B', 'main', 'load_fast' if fastB and full else 'load_fast_masked' if fastB and k4B else 'load'))
        for s, xk in enumerate(c.extras):
            if xk <= 0 or r.kernel == 'shortk':
                continue
            va, vb, kx4 = p.xlda[s] % 4 == 0, p.xldb[s] % 4 == 0, xk % 4 == 0 and xk >= 4
            out.add(('A', 'extra', 'load_fast_masked' if va and ((m % 4 == 0 and m >= 4) if c.tA else kx4) else 'load'))
            out.add(('B', 'extra', 'load_fast_masked' if vb and (kx4 if c.tB else (c.N % 4 == 0 and c.N >= 4)) else 'load'))
    return out


def fixup_loops(S):
    """k_gemm_fixup on S slabs: (passes of four, slabs of the remainder loop)."""
    return (S - 1) // 4, (S - 1) % 4


# ------------------------------------------------------------------------------------------------ inputs
def _gen(rng, family, shape, wide=False):
    if family == 'ints':
        lim = 8 if wide else 3
        v = rng.randint(-lim, lim + 1, size=shape)
        if v.size < 8:                               # a lone element must not be the zero that hides a dropped term
            v = np.where(v == 0, 2, v)
        return torch.from_numpy(v.astype(np.float32))
    v = (1.0 + 0.25 * rng.rand(*shape)) * np.where(rng.rand(*shape) < 0.5, -1.0, 1.0)
    return torch.from_numpy(v.astype(np.float32)).clamp(-1.25, 1.25)


_DATA, _REFS = collections.OrderedDict(), collections.OrderedDict()
_CACHE_ELEMS, _CACHE_ENTRIES = 1 << 21, 16        # (the last few cases only: the tests of a module come case after case or share seeds)


def _keep(cache, key, value, elems):
    if elems <= _CACHE_ELEMS:
        cache[key] = value
        while len(cache) > _CACHE_ENTRIES:
            cache.popitem(last=False)
    return value


def data(c, family):
    """The logical operands per batch item: Bag(A [m, k], B [k, N], xA [s][m, xK], xB [s][xK, N], C0 [m, N] as lists over items, bias)."""
    key = (c.seed, family)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.RandomState(zlib.crc32(('%s/%s' % (c.seed, family)).encode()) & 0x7fffffff)
    d = Bag(A=[], B=[], xA=[], xB=[], C0=[], bias=_gen(rng, family, (c.N,), True) if c.bias else None)
    for m, k in items(c):
        d.A.append(_gen(rng, family, (m, k)))
        d.B.append(_gen(rng, family, (k, c.N)))
        d.xA.append([_gen(rng, family, (m, xk)) for xk in c.extras])
        d.xB.append([_gen(rng, family, (xk, c.N)) for xk in c.extras])
        d.C0.append(_gen(rng, family, (m, c.N), True))
    return _keep(_DATA, key, d, sum(m * c.N for m, _ in items(c)))


def piece_tiles(c, k):
    """The k-tile sequence of an item: [(k index range in the concatenated reduction)] -- main pair, then each extra segment."""
    seq, base = [], 0
    for length in (k,) + tuple(c.extras):
        seq += [(base + t * BK, base + min(length, (t + 1) * BK)) for t in range(_cdiv(length, BK))]
        base += length
    return seq


def product(c, d, mut=None, with_terms=False):
    """The operator in float64, item by item, from the logical operands.  mut: one of the mutations of ``MUTATIONS`` (a wrong result
    of the kind a subtly broken kernel would produce).  -> [Bag(want, terms, ktot)]"""
    out = []
    nb = len(d.A)
    for b, (m, k) in enumerate(items(c)):
        Bsrc = (b + 1) % nb if mut == 'next B' else b
        xB = list(d.xB[b])
        A = torch.cat([d.A[b]] + d.xA[b], 1).double()
        if mut == 'swap xB' and len(xB) == 2:
            km = min(c.extras)
            x0, x1 = xB[0].clone(), xB[1].clone()
            x0[:km], x1[:km] = xB[1][:km], xB[0][:km]
            xB = [x0, x1]
        Bm = torch.cat([d.B[Bsrc]] + xB, 0).double()
        kk = A.shape[1]
        ks = list(range(kk))
        if mut == 'drop main last' and k >= 1:
            ks.remove(k - 1)
        if mut == 'drop extra first' and c.extras and c.extras[-1] > 0:
            ks.remove(k + sum(c.extras[:-1]))
        if mut == 'twice' and kk >= 1:
            ks.append(kk // 2)
        if mut == 'drop tile' and c.route.S > 1:
            seq = piece_tiles(c, k)
            if len(seq) >= 2:
                lo, hi = seq[max(len(seq) * 1 // c.route.S, 1)]
                ks = [i for i in ks if not lo <= i < hi]
        ks = torch.tensor(ks, dtype=torch.long)
        A, Bm = A[:, ks], Bm[ks]
        want = c.alpha * (A @ Bm)
        terms = abs(c.alpha) * (A.abs() @ Bm.abs()) if with_terms else None
        if d.bias is not None and mut != 'no bias':
            want = want + d.bias.double()
            terms = terms + d.bias.double().abs() if with_terms else None
        if c.beta != 0.0 and mut != 'no beta':
            want = want + c.beta * d.C0[b].double()
            terms = terms + abs(c.beta) * d.C0[b].double().abs() if with_terms else None
        if c.beta == 0.0 and mut == 'read C':
            want = want + float('nan')
        if mut == 'shift columns' and c.N > 4:
            want = torch.roll(want, 4, 1)
        if mut == 'shift rows' and m > 1:
            want = torch.roll(want, 1, 0)
        out.append(Bag(want=want, terms=terms, ktot=ktot(c, k)))
    return out


MUTATIONS = ('drop main last', 'drop extra first', 'twice', 'drop tile', 'swap xB', 'shift columns', 'shift rows', 'no bias', 'no beta',
             'read C', 'next B')


def applies(c, mut):
    it = [(m, k) for m, k in items(c) if m > 0]
    if not it or c.N <= 0:
        return False
    return {'drop main last': any(k >= 1 for _, k in it), 'drop extra first': bool(c.extras) and c.extras[-1] > 0,
            'twice': any(ktot(c, k) >= 1 for _, k in it),
            'drop tile': c.route.S > 1 and any(len(piece_tiles(c, k)) >= 2 for _, k in it),
            'swap xB': len(c.extras) == 2 and min(c.extras) > 0, 'shift columns': c.N > 4 and any(ktot(c, k) for _, k in it),
            'shift rows': any(m > 1 and ktot(c, k) for m, k in it), 'no bias': c.bias, 'no beta': c.beta != 0.0, 'read C': c.beta == 0.0,
            'next B': c.ragged == 1 and sum(1 for m, _ in it) >= 2 and c.K >= 1}[mut]


def reference(c, family):
    key = (c.seed, family)
    if key in _REFS:
        return _REFS[key]
    ref = product(c, data(c, family), with_terms=True)
    return _keep(_REFS, key, ref, sum(r.want.numel() for r in ref))


def magnitudes_ok(c):
    """'ints': every partial sum stays an exact float32 integer; 'reals': a single missing summand exceeds its element's allowance."""
    kmax = max([ktot(c, k) for _, k in items(c)] or [0])
    assert 2 * 9 * kmax + 24 < 2 ** 24
    assert kmax == 0 or (kmax + SLACK) * U32 * 1.5625 * kmax < 1
    # ... and with this case's alpha, beta and bias: the largest allowance is below the smallest summand |alpha| * 1 * 1
    worst = (kmax + SLACK) * U32 * (abs(c.alpha) * 1.5625 * kmax + 1.25 * (1 if c.bias else 0) + 1.25 * abs(c.beta))
    assert kmax == 0 or worst < abs(c.alpha)
    return True


def judge(c, family, got, ref):
    """got: [m, N] float32 per item.  -> Bag(excess, equal, rms): the largest error / allowance (inf: non-finite, or nonzero where terms
    is zero), whether got equals the reference as values, and the rms of err / terms over the elements with terms > 0."""
    worst, equal, sq, cnt = 0.0, True, 0.0, 0
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        g = g.detach().double().cpu()
        assert g.shape == r.want.shape, (g.shape, r.want.shape)
        if g.numel() == 0:
            continue
        if not bool(torch.isfinite(g).all()):
            return Bag(excess=float('inf'), equal=False, rms=float('inf'))
        equal = equal and bool((g == r.want).all())
        zero = r.terms == 0
        if bool((g[zero] != 0).any()):
            worst = float('inf')
        if not bool(zero.all()):
            err = (g - r.want).abs()[~zero]
            worst = max(worst, float((err / ((r.ktot + SLACK) * U32 * r.terms[~zero])).max()))
            sq += float(((err / r.terms[~zero]) ** 2).sum())
            cnt += int((~zero).sum())
    return Bag(excess=worst, equal=equal, rms=(sq / cnt) ** 0.5 if cnt else 0.0)


def chain_rms(c, d, ref, limit=1 << 20):
    """The rms of err / terms of a sequential float32 chain (s = fl(s + fl(a * b)), k ascending through the main pair and the extra
    segments, then fl(alpha * s), + bias, + fl(beta * C0)) on the same inputs -- the bar of the GPU file for 'reals'.  Items with more
    than ``limit`` elements in all are sampled by rows (every step-th row)."""
    total = sum(r.want.numel() for r in ref)
    step = max(1, _cdiv(total, limit))
    sq, cnt = 0.0, 0
    for b, r in enumerate(ref):
        if r.want.numel() == 0:
            continue
        A = torch.cat([d.A[b]] + d.xA[b], 1)[::step].contiguous()
        Bm = torch.cat([d.B[b]] + d.xB[b], 0)
        s = torch.zeros(A.shape[0], c.N)
        for k in range(A.shape[1]):
            s = s + A[:, k:k + 1] * Bm[k:k + 1]
        s = np.float32(c.alpha) * s
        if d.bias is not None:
            s = s + d.bias
        if c.beta != 0.0:
            s = s + np.float32(c.beta) * d.C0[b][::step]
        t = r.terms[::step]
        nz = t > 0
        sq += float((((s.double() - r.want[::step])[nz] / t[nz]) ** 2).sum())
        cnt += int(nz.sum())
    return (sq / cnt) ** 0.5 if cnt else 0.0


# ------------------------------------------------------------------------------------------------ placement on a device
class Places(object):
    """Operands in NaN-filled allocations, outputs in canary-filled ones (two spare rows before and after, padding columns, gaps);
    ``check()`` asserts that every float outside the logical elements of an output holds the bits it had before the launch."""

    def __init__(self, dev):
        self.dev, self.watch = dev, []

    def lay(self, mats, ld, stride, mis, fill, spare_rows=0):
        """mats: the stored [rows, width] matrix of every item; stride 0: consecutive row blocks.  -> Bag(view: 1-D from the base, pos)"""
        pos, at = [], 0
        for i, m in enumerate(mats):
            pos.append(at if stride == 0 else i * stride)
            at += m.shape[0] * ld
        total = (max(p + m.shape[0] * ld for p, m in zip(pos, mats)) if mats else 0)
        lead = up4(spare_rows * ld) + 4
        off = lead + (1 if mis else 0)
        cpu = torch.full((off + total + spare_rows * ld + 8,), fill, dtype=torch.float32)
        logical = torch.zeros(cpu.numel(), dtype=torch.bool)
        for p, m in zip(pos, mats):
            rows, width = m.shape
            if rows and width:
                cpu[off + p:off + p + rows * ld].view(rows, ld)[:, :width] = m
                logical[off + p:off + p + rows * ld].view(rows, ld)[:, :width] = True
        t = cpu.clone().to(self.dev)
        assert t.data_ptr() % 16 == 0
        return Bag(t=t, view=t[off:], off=off, pos=pos, ld=ld, shapes=[tuple(m.shape) for m in mats], logical=logical, before=cpu)

    def inp(self, mats, ld, stride, mis=False):
        return self.lay(mats, ld, stride, mis, float('nan'))

    def out(self, mats, ld, stride, mis=False):
        o = self.lay(mats, ld, stride, mis, CANARY, spare_rows=2)
        self.watch.append(o)
        return o

    def vec(self, t, dtype=torch.float32):
        return None if t is None else t.to(dtype).clone().to(self.dev)

    @staticmethod
    def items_of(o):
        """The logical [rows, width] matrices of a buffer, on the CPU."""
        flat = o.t.detach().cpu()
        return [flat[o.off + p:o.off + p + r * o.ld].view(r, o.ld)[:, :w].clone() for p, (r, w) in zip(o.pos, o.shapes)]

    def check(self):
        for o in self.watch:
            now = o.t.detach().cpu()
            keep = ~o.logical
            assert torch.equal(now[keep].view(torch.int32), o.before[keep].view(torch.int32)), 'a kernel wrote outside its output'


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def run(Kn, P, c, d):
    """One launch of case c on kernels Kn with the operands d.  -> the output buffer (Places.items_of gives its items)."""
    p, a = placement(c), call_args(c)
    T = lambda m: m.t().contiguous()
    A = P.inp([T(x) if c.tA else x for x in d.A], p.lda, p.sA, not p.alA)
    B = P.inp([T(x) if c.tB else x for x in d.B], p.ldb, p.sB, not p.alB)
    nan = float('nan')
    C = P.out([x if c.beta != 0.0 else torch.full_like(x, nan) for x in d.C0], p.ldc, p.sC, not p.alC)
    extra = []
    for s, xk in enumerate(c.extras):
        xa = P.inp([T(x[s]) if c.tA else x[s] for x in d.xA], p.xlda[s], p.xsA[s])
        xb = P.inp([T(x[s]) if c.tB else x[s] for x in d.xB], p.xldb[s], p.xsB[s])
        extra.append((xa.view, xb.view, p.xlda[s], p.xldb[s], xk, p.xsA[s], p.xsB[s]))
    for _ in range(a.fake_extras):                          # (invalid calls: never read)
        extra.append((A.view, B.view, p.lda, p.ldb, 8, 0, 0))
    gptr = None
    if c.ragged in (1, 2):
        gptr = P.vec(torch.tensor(np.concatenate([[0], np.cumsum(c.counts)])), torch.int32)
    Kn.gemm(A.view, B.view, C.view, a.M, a.N, a.K, a.tA, a.tB, p.lda, p.ldb, p.ldc, c.alpha, c.beta, P.vec(d.bias), a.batch, p.sA, p.sB,
            p.sC, gptr, a.ragged, a.max_ragged, int(sum(c.counts)), extra=extra)
    return C


def check_case(Kn, c, launch, families=('ints', 'reals'), with_chain=False):
    """Both families of a case: ``launch(run)`` calls run(Places) -> output buffer (the GPU file launches twice and asserts containment
    and identical bits).  -> (Excess keyed '<kernel> <family>', {family: Bag(excess, equal, rms, chain, outs)})"""
    ex, res = Excess(), {}
    for fam in families:
        d, ref = data(c, fam), reference(c, fam)
        o = launch(lambda P: run(Kn, P, c, d))
        got = Places.items_of(o)
        j = judge(c, fam, got, ref)
        j.outs, j.buf = got, o
        j.chain = chain_rms(c, d, ref) if with_chain and fam == 'reals' else None
        if with_chain and fam == 'reals' and j.chain is not None:
            total = sum(r.want.numel() for r in ref)
            step = max(1, _cdiv(total, 1 << 20))
            if step > 1:                                   # the kernel's rms on the rows the chain was computed on
                j.rms = judge(c, fam, [g[::step] for g in got], [Bag(want=r.want[::step], terms=r.terms[::step], ktot=r.ktot)
                                                                  for r in ref]).rms
        ex.add('%s %s' % (c.route.kernel, fam), j.excess)
        res[fam] = j
    return ex, res


def reduce_parts_check(Kn, P, c, buf, family):
    """ragged 3: cgc_reduce_batched over the parts of the (tight) output buffer against X^T dY over the whole K.  -> excess"""
    d, ref = data(c, family), reference(c, family)
    parts, numel = c.batch // c.outer, c.M * c.N
    out = P.out([torch.full((c.outer, numel), float('nan'))], numel, 0)
    Kn.reduce_batched(buf.view[:c.batch * numel], out.view[:c.outer * numel], c.outer, parts, numel, 0.0)
    got = Places.items_of(out)[0]
    worst = 0.0
    for o in range(c.outer):
        rs = ref[o * parts:(o + 1) * parts]
        want, terms = sum(r.want for r in rs).reshape(-1), sum(r.terms for r in rs).reshape(-1)
        g = got[o].double()
        if not bool(torch.isfinite(g).all()):
            return float('inf')
        if family == 'ints' and not bool((g == want).all()):
            return float('inf')
        worst = max(worst, float(((g - want).abs() / ((c.K + SLACK + parts + 2) * U32 * terms)).max()))
    return worst


# ------------------------------------------------------------------------------------------------ case list
REMAINDERS = (0, 1, 7, 8, 9, 24, 25, 31)
S_OF_KT = {6: 2, 12: 4, 15: 5, 24: 8, 27: 9, 36: 12}
TAIL_GRAPHS = (300, 0, 513, 128, 77, 1, 250, 640)


def d_counts(nb):
    """<= 200 rows per graph; empty graphs first, last and two in a row; a 1-row graph; three graphs (and more) of 64 rows."""
    if nb == 5:
        return (0, 1, 130, 0, 0)
    cyc = (64, 1, 64, 0, 0, 64, 200, 37, 130, 9)
    return (0,) + tuple(cyc[i % len(cyc)] for i in range(nb - 2)) + (0,)


def _cases():
    out = []

    def add(name, lay, M, N, K, **kw):
        kw.setdefault('ep', len(out))
        out.append(case(name, lay, M, N, K, **kw))
    odd, lays = dict(ldA='odd', ldB='odd'), tuple(LAYOUTS)
    # A: every instance
    for t in range(1, 7):
        BM, BN = tile_dims(t)
        M, N = BM + 37, BN + 21
        for lay in lays:
            for tag, K, kw in (('fit', 180, {}), ('fit', 181, {}), ('fit', 183, {}), ('odd', 181, odd), ('misA', 183, dict(mis=('A',))),
                               ('misB', 181, dict(mis=('B',))), ('ldcodd', 181, dict(ldC='odd')), ('misC', 183, dict(mis=('C',)))):
                add('A-c%d-%s-K%d-%s' % (10 + t, lay, K, tag), lay, M, N, K, cfg=10 + t, split=False, **kw)
            add('A-c%d-%s-K181-ldcodd-split' % (10 + t, lay), lay, M, N, 181, cfg=10 + t, ldC='odd')
            for tag, K, kw in (('fit', 41, {}), ('fit', 1, {}), ('odd', 41, odd), ('misA', 1, dict(mis=('A',))), ('misB', 41, dict(mis=('B',))),
                               ('misC', 41, dict(mis=('C',))), ('ldcodd', 1, dict(ldC='odd'))):
                add('A-c%d-%s-K%d-%s' % (20 + t, lay, K, tag), lay, M, N, K, cfg=20 + t, **kw)
    # B: K remainders at the k-group edges
    for i, lay in enumerate(lays):
        for r in REMAINDERS:
            for K in (r, 64 + r):
                if K == 0:
                    continue
                add('B-c%d-%s-K%d-fit' % (11 + i, lay, K), lay, 70, 45, K, cfg=11 + i, split=False)
                add('B-c%d-%s-K%d-odd' % (11 + i, lay, K), lay, 70, 45, K, cfg=11 + i, split=False, **odd)
                add('B-c%d-%s-K%d-fit' % (24 + i, lay, K), lay, 70, 45, K, cfg=24 + i)
    # C: tail split and fix-up
    for i, kt in enumerate(sorted(S_OF_KT)):
        add('C-S%d-%s' % (S_OF_KT[kt], lays[i % 3]), lays[i % 3], 100, 90, 32 * kt - 13, cfg=11)
    for t in range(2, 7):
        add('C-S5-c%d-%s' % (10 + t, lays[t % 3]), lays[t % 3], 150, 100, 467, cfg=10 + t)
    add('C-S5-c14-NN-ldcodd', 'NN', 150, 100, 467, cfg=14, ldC='odd', ep=1)
    add('C-xpiece-NT', 'NT', 100, 90, 180, extras=(40, 24), cfg=11, ep=1)
    add('C-T528-NT', 'NT', 505, 509, 200, batch=33, cfg=11, ep=1)
    add('C-T525-TN', 'TN', 377, 637, 200, batch=35, cfg=11, ep=2)
    add('C-raggedM-NN', 'NN', 0, 150, 200, ragged=1, counts=TAIL_GRAPHS, cfg=11, ep=1)
    add('C-raggedK-TN', 'TN', 150, 150, 0, ragged=2, counts=TAIL_GRAPHS, cfg=11, ep=0)
    # D: the TileMap modes without a tail
    for nb in (5, 8, 64, 65, 72):
        cnt = d_counts(nb)
        add('D-raggedM-NN-nb%d' % nb, 'NN', 0, 36, 70, ragged=1, counts=cnt, split=False)
        add('D-raggedM-NT-nb%d' % nb, 'NT', 0, 70, 36, ragged=1, counts=cnt, split=False)
        add('D-raggedK-TN-nb%d' % nb, 'TN', 70, 36, 0, ragged=2, counts=cnt, split=False)
    # E: ragged = 3
    for cfg in (0, 11):
        add('E-c%d-chunk128' % cfg, 'TN', 70, 45, 500, ragged=3, chunk=128, outer=2, cfg=cfg, ldC='tight', ep=0)
        add('E-c%d-chunk512' % cfg, 'TN', 70, 45, 500, ragged=3, chunk=512, outer=2, cfg=cfg, ldC='tight', ep=0)
    # F: extra K segments
    n = [0]

    def addx(name, lay, M, N, K, extras, **kw):
        n[0] += 1
        kw.setdefault('cfg', 0 if n[0] % 2 else 11 + n[0] % 6)
        add('F-%s-%s-x%s%s' % (name, lay, '+'.join(str(x) for x in extras), '-xodd' if kw.get('xodd') else ''), lay, M, N, K,
            extras=extras, **kw)
    for lay, M, N in (('NT', 100, 90), ('NN', 100, 92), ('TN', 102, 90)):
        addx('flat', lay, M, N, 100, (40,))
        addx('flat', lay, M, N, 100, (20, 24))
        addx('flat', lay, M, N, 100, (33,), xodd=(0,))
        addx('flat', lay, M, N, 100, (24, 33), xodd=(1,))
        addx('flat', lay, M, N, 100, (33, 24), xodd=(0,), split=False)
    addx('flat-M104', 'TN', 104, 90, 100, (24, 33), xodd=(1,))
    cnt = (37, 0, 130, 64)
    addx('raggedM', 'NT', 0, 90, 100, (40,), ragged=1, counts=cnt)
    addx('raggedM', 'NT', 0, 90, 100, (20, 24), ragged=1, counts=cnt)
    addx('raggedM', 'NT', 0, 90, 100, (33,), xodd=(0,), ragged=1, counts=cnt)
    addx('compaction', 'NT', 100, 90, 100, (0, 24))
    addx('compaction', 'NN', 100, 92, 100, (0, 24), cfg=12)
    for t in range(1, 7):
        addx('forced-shortk-c%d' % (20 + t), lays[t % 3], 100, 90, 41, (24,), cfg=20 + t)
    # G: degenerate and invalid
    for lay in lays:
        add('G-K0-%s-beta' % lay, lay, 70, 45, 0, ep=1)
        add('G-K0-%s-bias' % lay, lay, 70, 45, 0, ep=3)
        add('G-K0-%s-c11' % lay, lay, 70, 45, 0, ep=1, cfg=11)
        add('G-1x1x1-%s' % lay, lay, 1, 1, 1, ep=1)
    small = dict(ep=1)
    for name, kw, expect in (('N0', dict(N=0), 'noop'), ('batch0', dict(batch=0), 'noop'), ('M0', dict(M=0), 'noop'),
                             ('tAtB', dict(tA=True, tB=True), 'einval'), ('nx3', dict(fake_extras=3), 'einval'),
                             ('mode7', dict(mode=7), 'einval'), ('ragged4', dict(ragged=4), 'einval')):
        add('G-%s' % name, 'NN', 70, 45, 40, over=kw, expect=expect, ep=2)
    add('G-ragged1-tA', 'NN', 0, 36, 70, ragged=1, counts=(5, 9), over=dict(tA=True), expect='einval', **small)
    add('G-ragged2-extras', 'TN', 70, 36, 0, ragged=2, counts=(5, 9), over=dict(fake_extras=1), expect='einval', **small)
    add('G-ragged2-tB', 'TN', 70, 36, 0, ragged=2, counts=(5, 9), over=dict(tA=True, tB=True), expect='einval', **small)
    add('G-ragged3-batch', 'TN', 70, 45, 100, ragged=3, chunk=32, outer=2, over=dict(batch=7), expect='einval', ldC='tight', **small)
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert c.route.status == {'ok': 'launch'}.get(c.expect, c.expect), (c.name, c.route.status)
        assert c.expect != 'ok' or magnitudes_ok(c)
    return out


CASES = _cases()
VALID = [c for c in CASES if c.expect == 'ok']

# H: one logical product on every instance.  (tag, cfg, placement, with the extra segment)
H_SHAPE = (165, 149, 181, 24)


def h_cases(lay):
    """[(product 'x' (with the extra segment of 24) / 'plain', case)]: 6 tile shapes x {FAST, guarded} on both products, and the
    short-K kernel on the plain one; tail split off."""
    M, N, K, xk = H_SHAPE
    out = []
    for t in range(1, 7):
        for tag, kw in (('fast', {}), ('guarded', dict(ldA='odd', ldB='odd'))):
            out.append(('x', case('H-x-c%d-%s-%s' % (10 + t, lay, tag), lay, M, N, K, extras=(xk,), cfg=10 + t, split=False,
                                  seed='H-x-' + lay, **kw)))
            out.append(('plain', case('H-c%d-%s-%s' % (10 + t, lay, tag), lay, M, N, K, cfg=10 + t, split=False, seed='H-' + lay, **kw)))
        out.append(('plain', case('H-c%d-%s-shortk' % (20 + t, lay), lay, M, N, K, cfg=20 + t, split=False, seed='H-' + lay)))
    return out


# I: the reduce kernels
REDUCE_PARTS = (1, 6, 15, 16, 17, 63, 64, 65, 71, 72, 73, 129, 200)
REDUCE_NUMEL = (1, 31, 32, 33, 1000)
REDUCE_OUTER = (1, 3)
REDUCE_BETA = (0.0, 1.0, -0.5)
MANY_PARTS_FROM = 16          # cgc_reduce_batch_sum: parts >= 16 (and numel <= 2**20) -> k_reduce_many_parts


def reduce_kernel(entry, parts):
    return 'k_reduce_many_parts' if entry == 'batched' or parts >= MANY_PARTS_FROM else 'k_reduce_batch_sum'


def reduce_inputs(family, parts, numel, outer, beta):
    rng = np.random.RandomState(parts * 7919 + numel * 31 + outer)
    ws, out0 = _gen(rng, family, (outer, parts, numel)), _gen(rng, family, (outer, numel), True)
    want = ws.double().sum(1) + (beta * out0.double() if beta != 0.0 else 0.0)
    terms = ws.double().abs().sum(1) + abs(beta) * out0.double().abs()
    return Bag(ws=ws, out0=out0, want=want, terms=terms)


def run_reduce(Kn, P, r, entry, parts, numel, outer, beta):
    ws = P.inp([r.ws.reshape(outer * parts, numel)], numel, 0)
    out = P.out([r.out0 if beta != 0.0 else torch.full_like(r.out0, float('nan'))], numel, 0)
    if entry == 'batched':
        Kn.reduce_batched(ws.view[:outer * parts * numel], out.view[:outer * numel], outer, parts, numel, beta)
    else:
        assert outer == 1
        Kn.reduce_batch_sum(ws.view[:parts * numel], out.view[:numel], parts, numel, beta)
    return out


def judge_reduce(family, r, parts, got):
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return float('inf')
    if family == 'ints':
        return 0.0 if bool((g == r.want).all()) else float('inf')
    return float(((g - r.want).abs() / ((parts + 2) * U32 * r.terms)).max())
