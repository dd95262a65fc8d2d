"""CPU: the max-readout reference of tests/segmax_ref.py -- that its restated launch is the one in csrc/rowops.hip, that the case list
reaches every lane layout, both scans and every column group, that the prescribed columns land where their names say, that the
reference is torch.max over the dense padded tensor, and that the exact comparison rejects every mutant wherever it can show."""
import numpy as np
import pytest
import torch

import segmax_ref as S


def test_constants_are_the_sources():
    waves, ladder, wide, ahead, unroll = S.source_constants()
    assert (waves, wide, ahead, unroll) == (16, 64, 3, 4)
    assert ladder == ((2, 2), (4, 4), (8, 8), (16, 16), (32, 32))
    assert [S.route(D, 0).dp for D in S.WIDTHS] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64]
    assert S.route(20, 0).stride == 32 and S.route(8, 0).stride == 128 and S.route(2, 0).stride == 512
    assert [S.route(D, 0).groups for D in (64, 65, 130)] == [1, 2, 3]
    assert max(max(S.batch_counts(D)) * D for D in S.WIDTHS if S.route(D, 0).dp == 2) == 4099 * 2


def test_every_route_is_reached():
    seen = S.coverage()
    want = {(dp, unrolled, 0) for dp in (2, 4, 8, 16, 32, 64) for unrolled in (False, True)}
    want |= {(64, unrolled, g) for unrolled in (False, True) for g in (1, 2)}
    assert seen == want
    for D in S.WIDTHS:                                   # both sides of the unrolled scan's threshold, and the batch's empty graphs
        s, counts = S.route(D, 0).stride, S.batch_counts(D)
        assert not S.route(D, 3 * s).unrolled and S.route(D, 3 * s + 1).unrolled and {3 * s, 3 * s + 1} <= set(counts)
        assert counts[0] == 0 and counts[-1] == 0 and (0, 0) in zip(counts, counts[1:]) and sorted(set(counts)) == sorted(S.graph_sizes(D))
    for c in S.CASES:
        i = S.inputs(c)
        assert i.nmax == max(i.counts) + int(c.padded) and int(i.gptr[0]) == S.LEAD and i.n == int(i.gptr[-1]) + S.TRAIL


def test_prescribed_columns_cover_every_width_class():
    """Every prescription applies somewhere in every dp class, padded and not; the ties sit where their names say."""
    where = {}
    for c in S.CASES:
        i = S.inputs(c)
        for (b, _), p in i.placed.items():
            where.setdefault(p, set()).add((S.route(c.D, 0).dp, i.counts[b] < i.nmax))
    for p in S.PRESCRIPTIONS:
        dps = (2, 4, 8, 16, 32) if p == 'tie_subrows' else (2, 4, 8, 16, 32, 64)      # a full-wave row has no sub-rows
        assert where[p] >= {(dp, pad) for dp in dps for pad in (False, True)}, p
    for D in S.WIDTHS:
        r = S.route(D, 0)
        rows = 8 * r.stride + 3
        for p in S.TIES:
            col = np.zeros(rows, dtype=np.float32)
            if not S.PRESCRIPTIONS[p](col, D):
                assert p == 'tie_subrows' and r.rpw == 1
                continue
            a, b = (int(v) for v in np.nonzero(col)[0])
            (sa, ja), (sb, jb) = S.slot_of(D, a), S.slot_of(D, b)
            ua, ub = ja < S.unrolled_rows(D, rows, sa), jb < S.unrolled_rows(D, rows, sb)
            wave = lambda slot: slot // r.rpw
            if p == 'tie_unrolled_adjacent':
                assert sa == sb and jb == ja + 1 and ua and ub and ja // 4 == jb // 4
            elif p == 'tie_unrolled_remainder':
                assert sa == sb and jb == ja + 1 and ua and not ub
            elif p == 'tie_subrows':
                assert wave(sa) == wave(sb) and sb == sa + 1
            elif p == 'tie_waves':
                assert wave(sa) != wave(sb) and sa != 0 and sb != 0
            elif p == 'tie_merging_lane_first':
                assert sa == 0 and sb != 0
            else:                                        # the earlier row merges later: the `i < idx` branch
                assert sa > sb and a < b and (sb == 0) == (p == 'tie_merging_lane_later')


def _dense_max(c, dtype=torch.float64):
    """torch.max over dim 1 of the dense padded tensor (the reference model's readout) -> (values, indices)."""
    dense = torch.zeros(c.B, c.nmax, c.D, dtype=dtype)
    for b, cnt in enumerate(c.counts):
        lo = int(c.gptr[b])
        dense[b, :cnt] = torch.from_numpy(c.x[lo:lo + cnt].copy()).to(dtype)
    return dense.max(dim=1)


@pytest.mark.parametrize('D', S.WIDTHS)
def test_the_reference_is_torch_max_over_the_padded_tensor(D):
    for c in (c for c in S.CASES if c.D == D):
        i = S.inputs(c)
        out, arg = S.reference(c)
        val, idx = _dense_max(i, torch.float32)
        assert S.same_bits(out, val.numpy()), c.name
        for b, cnt in enumerate(i.counts):               # torch's index -> flat row, -1 where it points at padding
            want = np.where(idx[b].numpy() < cnt, int(i.gptr[b]) + idx[b].numpy(), -1)
            assert np.array_equal(arg[b], want), (c.name, b)
        assert S.judge_forward(c, out, arg) == []


def test_contract_examples():
    x = np.array([[1., -1., S.NAN, -S.INF, -0.0, S.INF], [1., -2., 5., -S.INF, -3., S.INF], [0., -3., S.NAN, -S.INF, -0.0, 2.]], dtype=np.float32)
    gptr = np.array([0, 3, 3], dtype=np.int32)
    out, arg = S.segment_max(x, gptr, 2, 6, 3)
    assert arg.tolist() == [[0, 0, 0, 0, 0, 0], [-1] * 6] and np.signbit(out[0, 4]) and out[0, 3] == -S.INF and np.isnan(out[0, 2])
    assert out[0, [0, 1, 5]].tolist() == [1., -1., S.INF] and not out[1].any()
    out, arg = S.segment_max(x, gptr, 2, 6, 4)
    assert arg[0].tolist() == [0, -1, 0, -1, 0, 0] and out[0, [0, 1, 3]].tolist() == [1., 0., 0.] and np.signbit(out[0, 4])
    assert not np.signbit(out[0, 1]) and np.isnan(out[0, 2])


# which prescriptions (padded or not) a mutant must be caught on, wherever they were placed
SHOWS = {
    'last_max': lambda p, padded: p in S.TIES or p in ('inf_two', 'negzero_then_zero', 'zero_then_negzero'),
    'padding_wins_ties': lambda p, padded: padded and p in ('max_zero', 'max_negzero', 'negzero_then_zero', 'zero_then_negzero'),
    'nan_ignored': lambda p, padded: p in S.NAN_COLUMNS,
    'neginf_is_empty': lambda p, padded: p == 'neginf_all' and not padded,
    'negzero_sign_dropped': lambda p, padded: p in ('max_negzero', 'negzero_then_zero'),
}


@pytest.mark.parametrize('mutant', S.MUTANTS)
def test_mutants_are_rejected(mutant):
    hit = set()
    for c in S.CASES:
        i = S.inputs(c)
        out, arg = S.segment_max(i.x, i.gptr, i.B, i.D, i.nmax, mutant=mutant)
        bad = {(b, d) for b, d, _ in S.judge_forward(c, out, arg)}
        if mutant == 'boundary_off_by_one':              # the last non-empty graph reads the first of the rows nobody owns: 1e30
            beaten = S.NAN_COLUMNS + ('inf_two',)         # beats everything but a NaN and +inf
            must = {(i.B - 2, d) for d in range(i.D) if i.placed.get((i.B - 2, d)) not in beaten}
        else:
            must = {k for k, p in i.placed.items() if SHOWS[mutant](p, i.counts[k[0]] < i.nmax)}      # padded: per graph
        assert must <= bad, (c.name, sorted(must - bad))
        if must:
            hit.add(S.route(c.D, 0).dp)
    assert hit == {2, 4, 8, 16, 32, 64}


def test_backward_reference_and_masked_planes():
    c = S.CASES[-1]
    i = S.inputs(c)
    _, arg = S.reference(c)
    dx, full = S.backward_reference(c, arg)
    assert (full[:S.LEAD] == S.CANARY).all() and (full[int(i.gptr[-1]):] == S.CANARY).all() and not (dx[:S.LEAD] != 0).any()
    inner = slice(S.LEAD, int(i.gptr[-1]))
    assert S.same_bits(dx[inner], full[inner]) and np.count_nonzero(dx) == np.count_nonzero(arg >= 0)
    m = S.masked_arg(arg)
    assert (m[:, 0] == -1).all() and (m[i.B - 2] == -1).all() and i.counts[i.B - 2] == max(i.counts) and (m >= 0).any()
    # the scatter is the gradient of the dense max: autograd through torch.max on a tie-free case
    x = torch.from_numpy(i.x.copy()).double().requires_grad_(True)
    rows = [x[int(i.gptr[b]):int(i.gptr[b + 1])] for b in range(i.B)]
    dense = torch.stack([torch.cat([r, torch.zeros(i.nmax - r.shape[0], i.D, dtype=torch.float64)]) for r in rows])
    clean = [d for d in range(i.D) if all(i.placed.get((b, d), 'random') == 'random' for b in range(i.B))]
    assert clean
    (dense.max(dim=1).values[:, clean] * torch.from_numpy(i.dout[:, clean].copy()).double()).sum().backward()
    assert np.array_equal(x.grad.numpy()[:, clean], dx[:, clean].astype(np.float64))
