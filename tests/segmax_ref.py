"""Exact reference of the max readout (csrc/rowops.hip: k_segment_max_fwd, k_segment_max_bwd, k_segment_max_bwd_full) for
tests/test_segmax_ref_cpu.py and tests/test_segmax_gpu.py.  Nothing here rounds: every comparison is of bits (out, dx) or of integers
(arg).

The contract (stated at cgc_segment_max_fwd in include/cgc_hip.h) is torch.max over dim 1 of the dense padded [B, nmax, D] tensor,
with the index translated to a row of the flat layout: ``segment_max`` walks that layout slot by slot -- the real rows of a graph in
order, then a zero where the graph has fewer than nmax rows -- and keeps the FIRST maximum, a NaN counting as larger than everything.
  out[b, d]   the maximum over the real rows, and over one zero as well when hi - lo < nmax
  arg[b, d]   the first real row that attains it; -1 when the padding zero wins strictly or the graph is empty (out = 0 then)
  a real row that ties with the padding wins (it comes first); a real -0.0 then comes out as -0.0
  any NaN among the real rows: out = NaN, arg = the first NaN row, padded or not
  all real rows -inf: without padding out = -inf and arg = lo; with padding the zero wins, out = 0 and arg = -1
  +inf wins at its first occurrence
It does not use oracle/flat_ref.py.

``route`` restates the launch of k_segment_max_fwd with its constants read from the source text; ``slot_of`` / ``unrolled_rows`` say
which lane reads a row and in which of its two loops; the prescribed columns (PRESCRIPTIONS) place ties, signed zeros and special
values by those, never by literals.  MUTANTS are single subtle errors of the reference -- two of them are what the kernel did before
this file existed -- that the exact comparison has to reject."""
import collections
import functools
import os
import re

import numpy as np
import torch

from rowops_ref import CANARY, Bag, Place  # noqa: F401

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cgc-net_amd', 'csrc', 'rowops.hip')

WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130)
LEAD, TRAIL = 2, 3               # rows of x before gptr[0] and after gptr[B]: no graph owns them
OUTSIDE = 1.0e30                 # what those rows hold: larger than everything inside, so a scan that strays takes it
TOP = 9.0                        # a placed maximum: above every N(0, 1) draw of these sizes
NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------------------------------------ the launch, restated
@functools.lru_cache(maxsize=None)
def source_constants():
    """(waves, ladder, wide, ahead, unroll) from the text of rowops.hip: SEGMAX_WAVES; the dp ladder ((2, 2), (4, 4), ...) with its last
    rung and the full-wave default; `r + ahead * stride < hi; r += unroll * stride` of the unrolled scan."""
    with open(SOURCE) as f:
        text = f.read()
    waves = int(re.search(r'#define SEGMAX_WAVES (\d+)', text).group(1))
    body = text[text.index('void k_segment_max_fwd('):text.index('void k_segment_max_bwd(')]
    wide = int(re.search(r'int dp = (\d+);', body).group(1))
    line = re.search(r'if \(D <= (\d+)\) dp = (.*?);', body)
    ladder = [(int(a), int(b)) for a, b in re.findall(r'D <= (\d+) \? (\d+)', line.group(2))]
    ladder.append((int(line.group(1)), int(re.search(r': (\d+)$', line.group(2)).group(1))))
    loop = re.search(r'for \(; r \+ (\d+) \* stride < hi; r \+= (\d+) \* stride\)', body)
    assert re.search(r'dim3\(B, ceil_div\(D, 64\)\), dim3\(64 \* SEGMAX_WAVES\)', text), 'the launch shape changed'
    assert 'const int stride = SEGMAX_WAVES * rpw;' in body and 'int r = lo + wave * rpw + sub;' in body
    return waves, tuple(ladder), wide, int(loop.group(1)), int(loop.group(2))


Route = collections.namedtuple('Route', 'dp rpw stride groups unrolled')


def route(D, rows):
    """-> (dp lanes per row, rows per wave, stride of a lane's scan, 64-column groups, whether a graph of ``rows`` rows enters the
    unrolled scan: its first lane does when lo + ahead * stride < hi)."""
    waves, ladder, wide, ahead, _ = source_constants()
    dp = wide
    for bound, lanes in ladder:
        if D <= bound:
            dp = lanes
            break
    rpw = 64 // dp
    stride = waves * rpw
    return Route(dp, rpw, stride, -(-D // 64), rows > ahead * stride)


def slot_of(D, k):
    """Row k of a graph (0-based) is read by lane slot k % stride = wave * rpw + sub, as that lane's (k // stride)-th row.  The merge
    visits the slots in increasing order, starting from slot 0's own result."""
    r = route(D, 0)
    return k % r.stride, k // r.stride


def unrolled_rows(D, rows, slot):
    """How many of a lane's rows the unrolled scan takes (a multiple of the unroll factor); the rest go through the remainder loop."""
    _, _, _, ahead, unroll = source_constants()
    stride = route(D, 0).stride
    rounds, r = 0, slot
    while r + ahead * stride < rows:
        rounds, r = rounds + 1, r + unroll * stride
    return unroll * rounds


def graph_sizes(D):
    s = route(D, 0).stride
    return (0, 1, s - 1, s, s + 1, 3 * s, 3 * s + 1, 4 * s + 1, 8 * s + 3)


def batch_counts(D):
    """One batch per width: an empty graph first, two consecutive empty ones in the middle, one last."""
    z = graph_sizes(D)
    assert z[0] == 0
    return (0,) + z[1:5] + (0, 0) + z[5:] + (0,)


# ------------------------------------------------------------------------------------------------ prescribed columns
def _tie(col, a, b):
    if not 0 <= a < b < len(col):
        return False
    col[a] = col[b] = TOP
    return True


def _p_tie_unrolled_adjacent(col, D):
    """Same lane, adjacent slots of one unrolled round (slot 0's second and third row)."""
    s = route(D, 0).stride
    return unrolled_rows(D, len(col), 0) >= 3 and _tie(col, s, 2 * s)


def _p_tie_unrolled_remainder(col, D):
    """Same lane, the last row of the unrolled scan and the first of the remainder loop."""
    s, u = route(D, 0).stride, unrolled_rows(D, len(col), 0)
    return u > 0 and _tie(col, (u - 1) * s, u * s)


def _p_tie_subrows(col, D):
    """Same wave, neighbouring sub-rows (wave 1, sub-rows 0 and 1)."""
    rpw = route(D, 0).rpw
    return rpw > 1 and _tie(col, rpw, rpw + 1)


def _p_tie_waves(col, D):
    rpw = route(D, 0).rpw
    return _tie(col, 2 * rpw, 5 * rpw)


def _p_tie_merging_lane_first(col, D):
    """The earlier row in wave 0, sub-row 0 -- the lane that merges."""
    return _tie(col, 0, 3 * route(D, 0).rpw)


def _p_tie_merging_lane_later(col, D):
    """The later row is the merging lane's second row, the earlier one sits in wave 3: the `i < idx` branch."""
    r = route(D, 0)
    return _tie(col, 3 * r.rpw, r.stride)


def _p_tie_late_lane_earlier(col, D):
    """The earlier row in the last slot, the later one in slot 1, which merges first: the `i < idx` branch between two other lanes."""
    s = route(D, 0).stride
    return _tie(col, s - 1, s + 1)


def _negative(col):
    col[:] = -np.abs(col) - np.float32(0.5)


def _p_all_negative(col, D):
    _negative(col)
    return True


def _p_max_zero(col, D):
    _negative(col)
    col[len(col) // 2] = 0.0
    return True


def _p_max_negzero(col, D):
    _negative(col)
    col[len(col) // 2] = -0.0
    return True


def _p_negzero_then_zero(col, D):
    if len(col) < 2:
        return False
    _negative(col)
    col[0], col[len(col) - 1] = -0.0, 0.0
    return True


def _p_zero_then_negzero(col, D):
    if len(col) < 2:
        return False
    _negative(col)
    col[0], col[len(col) - 1] = 0.0, -0.0
    return True


def _p_nan_one(col, D):
    col[len(col) // 2] = NAN
    return True


def _p_nan_two(col, D):
    """Two NaNs, the earlier one in a lane that merges later where the graph is long enough."""
    s = route(D, 0).stride
    a, b = (s - 1, s + 1) if len(col) > s + 1 else (0, len(col) - 1)
    if not a < b:
        return False
    col[a] = col[b] = NAN
    return True


def _p_nan_after_inf(col, D):
    if len(col) < 2:
        return False
    col[0], col[len(col) - 1] = INF, NAN
    return True


def _p_nan_all(col, D):
    col[:] = NAN
    return True


def _p_neginf_all(col, D):
    col[:] = -INF
    return True


def _p_neginf_some(col, D):
    col[::3] = -INF
    return True


def _p_inf_two(col, D):
    if len(col) < 2:
        return False
    col[len(col) // 3] = col[len(col) - 1] = INF
    return True


def _p_random(col, D):
    return True


PRESCRIPTIONS = collections.OrderedDict((f.__name__[3:], f) for f in (
    _p_tie_unrolled_adjacent, _p_tie_unrolled_remainder, _p_tie_subrows, _p_tie_waves, _p_tie_merging_lane_first,
    _p_tie_merging_lane_later, _p_tie_late_lane_earlier, _p_all_negative, _p_max_zero, _p_max_negzero, _p_negzero_then_zero,
    _p_zero_then_negzero, _p_nan_one, _p_nan_two, _p_nan_after_inf, _p_nan_all, _p_neginf_all, _p_neginf_some, _p_inf_two, _p_random))
TIES = tuple(p for p in PRESCRIPTIONS if p.startswith('tie_'))
NAN_COLUMNS = ('nan_one', 'nan_two', 'nan_after_inf', 'nan_all')


def variants(D):
    """Column d of variant v carries prescription (v * D + d) mod P: over ceil(P / D) variants every graph of the batch sees every one."""
    return -(-len(PRESCRIPTIONS) // D)


Case = collections.namedtuple('Case', 'D variant padded')
Case.name = property(lambda c: 'w%d-v%d-%s' % (c.D, c.variant, 'padded' if c.padded else 'longest'))
CASES = tuple(Case(D, v, padded) for D in WIDTHS for v in range(variants(D)) for padded in (False, True))


@functools.lru_cache(maxsize=None)
def _data(D, variant):
    counts = batch_counts(D)
    gptr = np.cumsum((LEAD,) + counts).astype(np.int32)
    n = int(gptr[-1]) + TRAIL
    rs = np.random.RandomState([D, variant])
    x = rs.standard_normal((n, D)).astype(np.float32)
    x[:LEAD] = OUTSIDE
    x[int(gptr[-1]):] = OUTSIDE
    names = list(PRESCRIPTIONS)
    placed = {}                                                   # (graph, column) -> prescription, where it applied
    for b, cnt in enumerate(counts):
        lo = int(gptr[b])
        for d in range(D):
            p = names[(variant * D + d) % len(names)]
            col = x[lo:lo + cnt, d].copy()
            if cnt > 0 and PRESCRIPTIONS[p](col, D):
                x[lo:lo + cnt, d] = col
                placed[(b, d)] = p
    dout = rs.standard_normal((len(counts), D)).astype(np.float32)
    x.setflags(write=False), gptr.setflags(write=False), dout.setflags(write=False)
    return x, gptr, dout, placed


def inputs(case):
    """-> Bag(x [n, D] float32, gptr [B + 1] int32 with gptr[0] = LEAD, B, D, n, nmax, counts, dout [B, D], placed)."""
    x, gptr, dout, placed = _data(case.D, case.variant)
    counts = batch_counts(case.D)
    return Bag(case=case, x=x, gptr=gptr, dout=dout, placed=placed, counts=counts, B=len(counts), D=case.D, n=x.shape[0],
               nmax=max(counts) + (1 if case.padded else 0))


# ------------------------------------------------------------------------------------------------ the reference
MUTANTS = ('last_max', 'padding_wins_ties', 'nan_ignored', 'neginf_is_empty', 'boundary_off_by_one', 'negzero_sign_dropped')


def segment_max(x, gptr, B, D, nmax, mutant=None):
    """x [n, D] float32 numpy, gptr [B + 1] -> (out [B, D] float32, arg [B, D] int32): a plain loop over the slots of the dense padded
    layout.  Only the first padding slot is visited: the others hold the same zero and cannot beat it."""
    assert mutant is None or mutant in MUTANTS, mutant
    out = np.zeros((B, D), dtype=np.float32)
    arg = np.full((B, D), -1, dtype=np.int32)
    for b in range(B):
        lo, hi = int(gptr[b]), int(gptr[b + 1])
        if mutant == 'boundary_off_by_one' and hi > lo:
            hi += 1                                               # the scan runs one row into the next graph
        pad = int(gptr[b + 1]) - int(gptr[b]) < nmax
        if hi == lo:
            continue                                              # only padding: out = 0, arg = -1
        for d in range(D):
            col = x[lo:hi, d].tolist()
            best, at, nan = None, -1, False                       # at = -1 with best set: the padding zero holds the maximum
            for t, v in enumerate(col + ([0.0] if pad else [])):
                real = t < len(col)
                if v != v:
                    if mutant == 'nan_ignored':
                        continue
                    best, at, nan = v, lo + t, True
                    break                                         # the first NaN: nothing replaces it
                if mutant == 'neginf_is_empty' and v == -INF:
                    continue
                if best is None:
                    take = True
                elif not real and mutant == 'padding_wins_ties':
                    take = v >= best
                elif real and mutant == 'last_max':
                    take = v >= best
                else:
                    take = v > best
                if take:
                    best, at = v, (lo + t if real else -1)
            if best is None:                                      # a mutant skipped every slot: it sees an empty graph
                best, at = 0.0, -1
            if mutant == 'negzero_sign_dropped' and not nan:
                best = best + 0.0
            out[b, d], arg[b, d] = best, at
    return out, arg


def scatter(dout, arg, n, D, fill_rows=None, base=0.0):
    """dx [n, D]: dout at (arg, column), ``base`` elsewhere -- zero inside the rows fill_rows = (first, last) when given (the full
    backward writes them all and leaves the rest alone), zero everywhere otherwise."""
    dx = np.full((n, D), base, dtype=np.float32)
    if fill_rows is not None:
        dx[fill_rows[0]:fill_rows[1]] = 0.0
    else:
        dx[:] = 0.0
    B = arg.shape[0]
    for b in range(B):
        for d in range(D):
            if arg[b, d] >= 0:
                dx[arg[b, d], d] = dout[b, d]
    return dx


def masked_arg(arg):
    """The reference's arg plane with a whole column and a whole graph (the longest) switched to -1, for the backward kernels."""
    a = arg.copy()
    a[:, 0] = -1
    a[a.shape[0] - 2, :] = -1
    return a


@functools.lru_cache(maxsize=None)
def reference(case):
    c = inputs(case)
    out, arg = segment_max(c.x, c.gptr, c.B, c.D, c.nmax)
    out.setflags(write=False), arg.setflags(write=False)
    return out, arg


# ------------------------------------------------------------------------------------------------ judges
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """Equal float32 bit patterns, every NaN counting as one value (the kernel hands the input's NaN through; its payload is not
    part of the contract)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def judge_forward(case, out, arg):
    """-> list of (graph, column, prescription) where out or arg differ from the reference; empty when the result is right."""
    want, warg = reference(case)
    out, arg = np.asarray(out, dtype=np.float32), np.asarray(arg, dtype=np.int32)
    assert out.shape == want.shape and arg.shape == warg.shape
    nan = np.isnan(want)
    bad = (np.isnan(out) != nan) | (~nan & (bits(out) != bits(want))) | (arg != warg)
    placed = inputs(case).placed
    return [(int(b), int(d), placed.get((int(b), int(d)), 'random')) for b, d in zip(*np.nonzero(bad))]


def coverage():
    """{(dp, unrolled, column group)} over the graphs of every width."""
    seen = set()
    for D in WIDTHS:
        for cnt in batch_counts(D):
            r = route(D, cnt)
            for g in range(r.groups):
                seen.add((r.dp, r.unrolled, g))
    return seen


# ------------------------------------------------------------------------------------------------ the direct calls
def _t(a):
    return torch.from_numpy(np.array(a))                          # a copy: the cached inputs are read-only


def run_forward(k, P, case):
    """cgc_segment_max_fwd into canary-surrounded out and arg -> (out, arg) numpy after a synchronize."""
    c = inputs(case)
    x, gptr = P.inp(_t(c.x)), P.inp(_t(c.gptr))
    out, arg = P.out(c.B, c.D), P.out(c.B, c.D, dtype=torch.int32)
    k.segment_max_fwd(x, gptr, c.B, c.D, c.nmax, out, arg)
    torch.cuda.synchronize()
    return out.cpu().numpy(), arg.cpu().numpy()


def run_backward(k, P, case, arg):
    """cgc_segment_max_bwd into a zeroed buffer and cgc_segment_max_bwd_full into a NaN-filled one whose rows before gptr[0] and after
    gptr[B] hold the canary, both inside Place's canaries -> (dx, dx_full) numpy."""
    c = inputs(case)
    dout, a, gptr = P.inp(_t(c.dout)), P.inp(_t(arg)), P.inp(_t(c.gptr))
    dx, full = P.out(c.n, c.D), P.out(c.n, c.D)
    dx.zero_()
    full[LEAD:int(c.gptr[-1])] = NAN
    k.segment_max_bwd(dout, a, c.B, c.D, dx)
    k.segment_max_bwd_full(dout, a, gptr, c.B, c.D, c.nmax, full)
    torch.cuda.synchronize()
    return dx.cpu().numpy(), full.cpu().numpy()


def backward_reference(case, arg):
    c = inputs(case)
    return (scatter(c.dout, arg, c.n, c.D), scatter(c.dout, arg, c.n, c.D, fill_rows=(LEAD, int(c.gptr[-1])), base=CANARY))
