"""CPU: the bookkeeping that the case list of tests/test_gemm_fp64_gpu.py (tests/gemm_ref.py) reaches all 54 instances of the exact fp32
GEMM, the six fix-up instances, every fix-up loop shape, both branches of TileMap::tail_slot, the three TileMap modes and every loader
sub-choice of the guarded kernel; the constants the restatement assumes, parsed from csrc/gemm.hip and csrc/gemm_common.hpp; the float32
restatement (oracle/flat_ref.TorchKernels.gemm), driven by the same code as the HIP kernels, equal on 'ints' and within the derived
allowance on 'reals' with the canaries intact on every case; and the sensitivity of the check -- each kind of subtly wrong result is
noticed on every case it applies to, in both input families."""
import os

import pytest

import gemm_ref as G
from oracle.flat_ref import TorchKernels

TWIN = TorchKernels()
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cgc-net_amd', 'csrc')
BY_NAME = {c.name: c for c in G.CASES}


def once(run):
    P = G.Places('cpu')
    o = run(P)
    P.check()
    return o


# ---------------------------------------------------------------------------------------------- bookkeeping over the case list
def test_case_list_reaches_every_instance_and_branch():
    """BOOKKEEPING: gemm_ref.dispatch() restates gemm_dispatch and has to follow it when it changes."""
    inst = {c.route.instance for c in G.VALID}
    want = {(t, k, lay) for t in G.TILES for k in ('fast', 'guarded', 'shortk') for lay in G.LAYOUTS}
    assert len(want) == 54 and not want - inst, 'not reached: %r' % sorted(want - inst)
    # ... each of them by a forced A case of its own tile shape, at the shape the case table prescribes
    for t in G.TILES:
        BM, BN = G.tile_dims(t)
        for lay in G.LAYOUTS:
            a = [c for c in G.VALID if c.name.startswith('A-c%d-%s-' % (10 + t, lay)) or c.name.startswith('A-c%d-%s-' % (20 + t, lay))]
            assert {c.route.kernel for c in a} == {'fast', 'guarded', 'shortk'}
            assert all((c.M, c.N) == (BM + 37, BN + 21) and c.route.tile == t for c in a)
            assert {c.K for c in a if c.route.kernel == 'fast'} >= {180, 181, 183} and {c.K for c in a if c.route.kernel == 'shortk'} == {41, 1}
            # the scalar epilogue over a whole tile: FAST operands with an odd ldc / a misaligned C, in the kernel and in the fix-up
            epi = {(c.ldC, c.mis, c.route.S > 1) for c in a if c.route.kernel == 'fast'}
            assert epi >= {('odd', (), False), ('fit', ('C',), False), ('odd', (), True)}
            assert all(c.route.S == 1 for c in a if not c.name.endswith('-split'))
    assert {G.TILES[t][3] for t in G.TILES} == {1, 2}
    # epilogue parameters: every (alpha, beta, bias) on every kernel kind
    for k in ('fast', 'guarded', 'shortk'):
        assert {(c.alpha, c.beta, c.bias) for c in G.VALID if c.route.kernel == k} == set(G.EPI)
    # fix-up: all six instances, every S of the table, the loop shapes
    split = [c for c in G.VALID if c.route.S > 1]
    assert {c.route.tile for c in split} == set(G.TILES)
    assert {c.route.S for c in split} >= {2, 3, 4, 5, 6, 8, 9, 12}
    assert {G.fixup_loops(c.route.S) for c in split} >= {(0, 1), (0, 3), (1, 0), (1, 3), (2, 0), (2, 3)}
    for kt, S in G.S_OF_KT.items():
        c = [c for c in G.VALID if c.name.startswith('C-S%d-' % S) and c.route.tile == 1][0]
        assert (c.M, c.N, c.K, c.route.T, c.route.L, c.route.S) == (100, 90, 32 * kt - 13, 1, 1, S)
    for t in range(2, 7):
        assert [c.route.S for c in G.VALID if c.name.startswith('C-S5-c%d' % (10 + t))][0] == 5
    x = BY_NAME['C-xpiece-NT']
    seq = G.piece_tiles(x, x.K)
    assert x.route.S == 3 and len(seq) == 9 and seq[6][0] == x.K          # the third piece [6, 9) holds extra segments only
    r = BY_NAME['C-T528-NT'].route
    assert (r.T, r.L, r.S, r.Tdp, r.slot_branches) == (528, 16, 2, 512, {1})
    r = BY_NAME['C-T525-TN'].route
    assert (r.T, r.L, r.S, r.T & 7, r.slot_branches) == (525, 13, 2, 5, {1, 2})
    assert {b for c in split for b in c.route.slot_branches} == {1, 2}
    # TileMap modes, with and without a tail; the plain cut with empty tiles at more than 64 graphs
    assert {(c.route.mode, c.route.S > 1) for c in G.VALID} >= {(m, s) for m in (0, 1, 2) for s in (False, True)}
    for nb in (5, 8, 64, 65, 72):
        modes = [BY_NAME['D-ragged%s-nb%d' % (k, nb)].route.mode for k in ('M-NN', 'M-NT', 'K-TN')]
        assert modes == [1 if nb <= 64 else 0, 1 if nb <= 64 else 0, 2 if nb in (8, 64) else 0]
        cnt = G.d_counts(nb)
        assert len(cnt) == nb and max(cnt) <= 200 and cnt[0] == 0 and cnt[-1] == 0 and 1 in cnt
        assert any(a == 0 and b == 0 for a, b in zip(cnt, cnt[1:]))
        assert nb == 5 or sum(1 for v in cnt if v == 64) >= 3
        assert all(BY_NAME['D-ragged%s-nb%d' % (k, nb)].route.S == 1 for k in ('M-NN', 'M-NT', 'K-TN'))
    for name in ('C-raggedM-NN', 'C-raggedK-TN'):
        assert BY_NAME[name].route.S > 1 and BY_NAME[name].counts == G.TAIL_GRAPHS
    # loader sub-choices of the guarded kernel's fetch lambda
    seen = set()
    for c in G.VALID:
        if c.route.kernel == 'guarded':
            seen |= G.fetch_choices(c)
    want = {(o, 'main', ld) for o in 'AB' for ld in ('load_fast', 'load_fast_masked', 'load')}
    want |= {(o, 'extra', ld) for o in 'AB' for ld in ('load_fast_masked', 'load')}
    assert not want - seen, sorted(want - seen)
    # K % 4 in {1, 3} through load_fast_masked of a k-contiguous operand: in the FAST kernel (fetch_seg) and in the guarded one
    ks = {(c.lay, c.K % 4) for c in G.VALID if c.route.kernel == 'fast' and c.name.startswith('A-')}
    assert ks >= {(lay, r) for lay in G.LAYOUTS for r in (0, 1, 3)}
    ks = {(o, c.K % 4) for c in G.VALID if c.route.kernel == 'guarded' for o in 'AB'
          if (o, 'main', 'load_fast_masked') in G.fetch_choices(c) and (c.tB if o == 'B' else not c.tA)}
    assert ks >= {('A', 1), ('B', 3)}, ks
    # K remainders: both kernels, every layout
    for i, lay in enumerate(G.LAYOUTS):
        for cfg, kern in ((11 + i, {'fast', 'guarded'}), (24 + i, {'shortk'})):
            b = [c for c in G.VALID if c.name.startswith('B-c%d-%s-' % (cfg, lay))]
            assert {c.route.kernel for c in b} == kern
            assert {c.K for c in b} == {r for r in G.REMAINDERS if r} | {64 + r for r in G.REMAINDERS}
    # extra segments: one and two, on FAST and guarded, in every form; the compaction; the forced short-K route keeps its segment
    f = [c for c in G.VALID if c.name.startswith('F-')]
    forms = {(c.lay, c.ragged, len(c.extras), c.route.kernel) for c in f}
    assert forms >= {(lay, 0, n, k) for lay in G.LAYOUTS for n in (1, 2) for k in ('fast', 'guarded')}
    assert {(len(c.extras), c.route.kernel) for c in f if c.ragged == 1 and c.lay == 'NT'} >= {(1, 'fast'), (2, 'fast'), (1, 'guarded')}
    assert any(c.extras[0] == 0 for c in f) and {x for c in f for x in c.extras} >= {0, 20, 24, 33, 40}
    assert any(c.lay == 'TN' and c.M % 4 for c in f)
    forced = [c for c in f if c.cfg >= 20]
    assert {c.cfg for c in forced} == set(range(21, 27)) and all(c.route.kernel != 'shortk' and c.route.tile == c.cfg - 20 for c in forced)
    # ragged = 3: 4 parts (the last of 116 rows) x 2 outer items, and one part; the automatic route and cfg 11
    e = BY_NAME['E-c0-chunk128']
    assert e.counts == (128, 128, 128, 116) * 2 and BY_NAME['E-c0-chunk512'].counts == (500, 500)
    assert {c.cfg for c in G.VALID if c.ragged == 3} == {0, 11}
    # invalid and empty calls
    assert sorted(c.name for c in G.CASES if c.expect == 'noop') == ['G-M0', 'G-N0', 'G-batch0']
    assert len([c for c in G.CASES if c.expect == 'einval']) == 8
    # H: every instance on both products, the short-K kernel on the plain one
    for lay in G.LAYOUTS:
        h = G.h_cases(lay)
        assert {(p, c.route.tile, c.route.kernel) for p, c in h} == (
            {(p, t, k) for p in ('x', 'plain') for t in G.TILES for k in ('fast', 'guarded')} | {('plain', t, 'shortk') for t in G.TILES})
        assert all(c.route.S == 1 and c.route.lay == lay for _, c in h)
        assert len({id(G.data(c, 'reals')) for p, c in h if p == 'x'}) == 1 and len({id(G.data(c, 'reals')) for p, c in h if p == 'plain'}) == 1
    assert G.reduce_kernel('sum', 15) == 'k_reduce_batch_sum' and G.reduce_kernel('sum', 16) == 'k_reduce_many_parts'


def test_restatement_assumes_the_constants_of_the_source():
    """A retune of a dispatch constant fails here instead of silently shrinking what the case list covers."""
    with open(os.path.join(CSRC, 'gemm.hip')) as f:
        hip = ' '.join(f.read().split())
    with open(os.path.join(CSRC, 'gemm_common.hpp')) as f:
        hpp = ' '.join(f.read().split())
    assert 'constexpr int shortk_max = %d, fill_min = %d;' % (G.SHORTK_MAX, G.FILL_MIN) in hip
    assert 'static const int kResident = %d;' % G.RESIDENT in hip and '#define BK %d' % G.BK in hpp
    assert 'const bool sk = k_extent <= shortk_max && a.nx == 0;' in hip
    assert 'const bool fsk = force >= 20 ? a.nx == 0 : force >= 10 ? false : sk;' in hip
    assert '(big || plan.tiles <= %d)) plan.tail_split(ws, ws_floats, %d, kResident);' % (G.SPLIT_TILES_MAX, G.MIN_KT) in hip
    assert 'const int s_max = (int)(kt / min_kt < %d ? kt / min_kt : %d);' % (G.S_CAP, G.S_CAP) in hpp
    assert 'unsigned s = (R + l / 2) / l;' in hpp and 'const unsigned l = T < R ? T : T % R;' in hpp
    assert 'if (a.ragged == 1 && nb <= 64) {' in hpp and '} else if (a.ragged == 2 && nb <= 64 && (nb & 7u) == 0) {' in hpp
    assert 'if (!sk && ws != nullptr && k_extent >= 24 * BK) return big_route(sk, ws);' in hip
    assert 'if (k_extent > 256 && m_extent > 128)' in hip
    for t, (wgm, wgn, tm, tn) in G.TILES.items():
        if t == 1:
            assert 'case 1: return big_route(fsk, ws);' in hip and 'return launch_cfg<2, 2, 2, 2>(a, transA' in hip
        else:
            assert 'case %d: return launch_cfg<%d, %d, %d, %d>(a, transA' % (t, wgm, wgn, tm, tn) in hip
    assert 'if (parts >= %d && numel <= (1 << 20)) return cgc_reduce_batched(' % G.MANY_PARTS_FROM in hip
    # a few values of the restatement itself
    a = G.case('probe', 'NN', 1140, 1140, 1140, batch=32)
    assert (a.route.tile, a.route.kernel, a.route.T, a.route.L, a.route.S) == (1, 'fast', 2592, 32, 12)
    assert G.case('probe', 'NN', 300, 20, 64).route.instance == (5, 'shortk', 'NN')
    assert G.case('probe', 'NT', 20, 300, 500).route.tile == 6 and G.case('probe', 'NT', 50, 300, 500).route.tile == 3
    assert G.case('probe', 'TN', 1140, 1140, 1800, batch=4).route.tile == 1
    assert G.case('probe', 'TN', 1140, 1140, 1800, batch=4, split=False).route.tile == 2


# ---------------------------------------------------------------------------------------------- the float32 restatement
@pytest.mark.parametrize('c', G.VALID, ids=lambda c: c.name)
def test_float32_restatement_passes(c):
    """The same driver as on the GPU, on the float32 torch restatement: 'ints' equal, 'reals' within the allowance, canaries intact."""
    assert G.magnitudes_ok(c)
    ex, res = G.check_case(TWIN, c, once)
    print('GEMM twin %s: %s' % (c.name, ex.line()))
    assert res['ints'].equal and res['ints'].excess == 0.0, c.name
    assert res['reals'].excess <= 1.0, (c.name, ex)
    if c.ragged == 3:
        for fam in ('ints', 'reals'):
            P = G.Places('cpu')
            assert G.reduce_parts_check(TWIN, P, c, res[fam].buf, fam) <= 1.0
            P.check()


@pytest.mark.parametrize('c', [c for c in G.CASES if c.expect == 'noop'], ids=lambda c: c.name)
def test_empty_calls_write_nothing_on_the_restatement(c):
    d = G.data(c, 'ints')
    P = G.Places('cpu')
    o = G.run(TWIN, P, c, d)
    assert G.same_bits(o.t, o.before)


def test_chain_and_reference_rounded_are_inside_the_allowance():
    """The sequential float32 chain that sets the rms bar, and the reference rounded to float32, pass the yardstick with room."""
    for name in ('A-c11-NN-K181-fit', 'C-S12-TN', 'F-flat-NT-x20+24', 'C-raggedK-TN'):
        c = BY_NAME[name]
        d, ref = G.data(c, 'reals'), G.reference(c, 'reals')
        j = G.judge(c, 'reals', [r.want.float() for r in ref], ref)
        assert j.excess <= 0.5 and 0 < G.chain_rms(c, d, ref) < 2.0 ** -20
        bad = [r.want.float().clone() for r in ref]
        bad[-1][-1, -1] = float('nan')
        assert G.judge(c, 'reals', bad, ref).excess == float('inf')
    c = BY_NAME['C-raggedK-TN']                      # the graph of K = 0: terms are zero, the result must be exactly zero
    ref = G.reference(c, 'reals')
    assert bool((ref[1].terms == 0).all())
    dirty = [r.want.float().clone() for r in ref]
    dirty[1][0, 0] = 1e-30
    assert G.judge(c, 'reals', dirty, ref).excess == float('inf')


# ---------------------------------------------------------------------------------------------- the check discriminates
@pytest.mark.parametrize('c', G.VALID, ids=lambda c: c.name)
def test_check_notices_every_mutation(c):
    applied = set()
    for fam in ('ints', 'reals'):
        d, ref = G.data(c, fam), G.reference(c, fam)
        for mut in G.MUTATIONS:
            if not G.applies(c, mut):
                continue
            applied.add(mut)
            got = [r.want.float() for r in G.product(c, d, mut)]
            j = G.judge(c, fam, got, ref)
            assert (not j.equal) if fam == 'ints' else j.excess > 1.0, '%s: not noticed on %s / %s' % (mut, c.name, fam)
    expect = {'read C'} if c.beta == 0.0 else {'no beta'}
    expect |= {'no bias'} if c.bias else set()
    expect |= {'drop extra first'} if c.extras and c.extras[-1] else set()
    expect |= {'swap xB'} if len(c.extras) == 2 and min(c.extras) > 0 else set()
    expect |= {'drop tile'} if c.route.S > 1 else set()
    expect |= {'next B'} if c.ragged == 1 else set()
    if max(k for _, k in G.items(c)) >= 1:
        expect |= {'drop main last', 'twice'}
    assert applied >= expect, (c.name, expect - applied)


def test_check_notices_a_written_canary():
    c = BY_NAME['A-c14-NN-K180-fit']
    d = G.data(c, 'ints')
    for where in ('padding', 'before', 'after'):
        P = G.Places('cpu')
        o = G.run(TWIN, P, c, d)
        P.check()
        i = {'padding': o.off + c.N, 'before': o.off - 1, 'after': o.t.numel() - 1}[where]
        assert not bool(o.logical[i])
        o.t[i] = 0.0
        with pytest.raises(AssertionError):
            P.check()


# ---------------------------------------------------------------------------------------------- the reduce kernels' restatement
@pytest.mark.parametrize('parts', G.REDUCE_PARTS)
def test_reduce_restatement_passes(parts):
    for numel in G.REDUCE_NUMEL:
        for outer in G.REDUCE_OUTER:
            for beta in G.REDUCE_BETA:
                for fam in ('ints', 'reals'):
                    r = G.reduce_inputs(fam, parts, numel, outer, beta)
                    for entry in ('batched',) + (('sum',) if outer == 1 else ()):
                        P = G.Places('cpu')
                        o = G.run_reduce(TWIN, P, r, entry, parts, numel, outer, beta)
                        P.check()
                        assert G.judge_reduce(fam, r, parts, G.Places.items_of(o)[0]) <= 1.0, (parts, numel, outer, beta, fam, entry)
                    wrong = r.want.clone()
                    p = int(r.ws[-1].abs().sum(1).argmax())                     # a part of the last outer item dropped
                    wrong[-1] -= r.ws[-1, p].double()
                    assert G.judge_reduce(fam, r, parts, wrong.float()) > 1.0
