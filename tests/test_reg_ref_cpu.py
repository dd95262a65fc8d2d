"""CPU: the regulariser reference of tests/reg_ref.py -- that its restated launches are the ones in csrc/diffpool_reg.hip, that the
cases reach every kernel instance and every loop's second pass, that the float64 reference is the formula it claims (against PyG's
dense_diff_pool expressions spelled out on dense tensors), that the float32 twins pass every judge, and that each mutant is rejected
on every case where it can show."""
import numpy as np
import pytest

import reg_ref as R


def test_constants_are_the_sources():
    k = R.source_constants()
    assert (k.block, k.parts, k.ent_bwd_cap, k.adj_bwd_cap, k.prep_cap) == (256, 512, 4096, 4096, 8192)
    assert R.grid_for(0, 512) == 1 and R.grid_for(257, 512) == 2 and R.grid_for(10 ** 9, 512) == 512


def test_every_route_is_reached():
    ent = {}
    for r in R.ROW_CASES:
        ro = R.route_rows(r.n, r.C, r.ld, r.off == 0)
        ent.setdefault(ro.vec, []).append((r, ro))
    assert [r for r, _ in ent[4]] == list(R.ROW_CASES[:3]) and len(ent[1]) == 6
    for vec in (4, 1):                                  # a second pass of the lane loop in both instances
        assert any(ro.lane_passes >= 2 for _, ro in ent[vec]) and any(ro.lane_passes == 1 for _, ro in ent[vec])
    assert R.route_rows(2100, 8, 8, True).row_passes == 2 and R.route_rows(2100, 8, 8, True).blocks == 512      # 2048 waves
    assert R.route_rows(2048, 8, 8, True).row_passes == 1
    why = {r: (r.C % 4 != 0, r.ld % 4 != 0, r.off != 0) for r, _ in ent[1]}                                   # every reason for <1>
    assert {w for w in why.values()} >= {(True, True, False), (False, False, True), (False, True, False)}
    cap = R.source_constants().ent_bwd_cap
    assert R.route_rows(16400, 4, 4, True, cap=cap).row_passes == 2 and R.route_rows(16384, 4, 4, True, cap=cap).row_passes == 1
    assert all(R.route_rows(r.n, r.C, r.ld, True, cap=cap).row_passes <= 1 for r in R.ROW_CASES)
    sq = {m: R.route_sumsq(m, True) for m in R.SUMSQ_M}
    assert sq[524295].vec_passes == 2 and sq[524295].tail == 3 and R.route_sumsq(524291, True).blocks == 512 and sq[1025].vec_passes == 1
    assert [sq[m].tail for m in R.SUMSQ_M] == [0, 1, 3, 0, 1, 3, 1, 3] and sq[3].vec_passes == 0 and sq[4].vec_passes == 1
    assert all(R.route_sumsq(m, False).vec_passes == 0 and R.route_sumsq(m, False).tail == m for m in R.SUMSQ_M)
    assert all(R.route_sumsq(nnz, True, csr=True).blocks == 512 for nnz in R.CSR_NNZ)
    assert [R.route_flat(m)[1] for m in R.ADJ_M] == [1, 1, 1, 2] and R.route_flat(257)[0] == 2
    assert [R.route_prep(B, C)[1:] for B, C in R.PREP_BC] == [(1, 1), (1, 1), (1, 2), (2, 1)]
    names = list(R.forward_cases())
    assert len(names) == len(R.ROW_CASES) + 2 * len(R.SUMSQ_M) + 3 * len(R.CSR_NNZ) + len(R.TRACE_BC) + len(R.FINALIZE)


def test_row_contents():
    S = R.rows_matrix(37, 5)
    assert (S[1] == 1).sum() == 1 and (S[1] == 0).sum() == 4 and not S[2].any() and (S[3] == np.float32(1) / np.float32(5)).all()
    assert np.float32(1e-30) in S[4] and np.float32(1e-15) in S[4] and abs(S[0].sum() - 1) < 1e-6


def test_the_reference_is_the_dense_formula():
    """link = ||A - S S^T||_F / numel and ent = mean row entropy on dense tensors, against the trace form the kernels use."""
    rs = np.random.RandomState(3)
    B, N, C = 2, 6, 3
    S = R.rows_matrix(B * N, C).astype(np.float64).reshape(B, N, C)
    A = rs.standard_normal((B, N, N))
    G = np.einsum('bnc,bnd->bcd', S, S)
    A_out = np.einsum('bnc,bnm,bmd->bcd', S, A, S)
    c = R.Bag(S=S.reshape(B * N, C).astype(np.float32), G=G, A_out=A_out, A=A.reshape(-1), rowptr=None, numel=float(B * N * N),
              rows_count=float(B * N))
    ref = R.forward(R.Bag(**{**c.__dict__, 'G': G.astype(np.float32), 'A_out': A_out.astype(np.float32), 'A': A.reshape(-1).astype(np.float32)}))
    link = np.sqrt(((A - np.einsum('bnc,bmc->bnm', S, S)) ** 2).sum()) / (B * N * N)
    ent = (-S * np.log(S + 1e-15)).sum(-1).mean()
    assert abs(ref.link - link) < 1e-6 * link and abs(ref.ent - ent) < 1e-12


def test_finalize_cases_are_what_they_claim():
    cs = R.forward_cases()
    for name, ratio in R.FINALIZE_RATIO.items():
        ref = R.forward(cs['finalize-' + name])
        assert ref.T / (ref.a2 + 2 * abs(ref.tr) + ref.g2) == pytest.approx(ratio, rel=1e-12) and ref.T > 0
    z, neg = R.forward(cs['finalize-zero']), R.forward(cs['finalize-negative'])
    assert z.T == 0 and z.a2 == z.g2 == z.tr == 4 and z.link == 0 and z.keep == 0
    assert neg.T < 0 and neg.link == 0 and neg.keep == 0
    for nnz in R.CSR_NNZ:                               # the CSR buffers hold NaN beyond nnz
        c = cs['csr-nnz%d-val' % nnz]
        assert int(c.rowptr[-1]) == nnz and len(c.A) == nnz + R.CSR_SPARE and np.isnan(c.A[nnz:]).all() and np.isfinite(c.A[:nnz]).all()
        assert (np.diff(c.rowptr) >= 0).all() and R.forward(cs['csr-nnz%d-ones' % nnz]).a2 == nnz


def _forward_excess(c, mutant=None):
    ex = R.Excess()
    R.judge_forward(c, R.forward(c), *R.twin_forward(c, mutant), ex)
    return ex


def test_twins_pass_every_judge():
    total = R.Excess()
    for name, c in R.forward_cases().items():
        ex = _forward_excess(c)
        assert all(e <= 1.0 for e in ex.values()), (name, ex)
        for k, e in ex.items():
            total.add(k, e)
    S = R.sweep()
    g, unit = R.ent_grad64(S)
    total.add('logf sweep (numpy float32), units', float((np.abs(R.twin_ent_grad(S).astype(np.float64) - g) / (R.U * unit)).max()))
    assert total['logf sweep (numpy float32), units'] <= R.LOGF_GRANTED and S.min() > 0 and S.max() == 1
    assert ((S > 0.9e-15) & (S < 1.1e-15)).sum() > 100
    for rows in R.ROW_CASES_BWD:
        S, ds0 = R.rows_matrix(rows.n, rows.C), R._rnd([rows.n, rows.C, 1], rows.n, rows.C)
        total.add('entropy_bwd', R.judge_entropy_bwd(S, -0.37, ds0, R.twin_entropy_bwd(S, -0.37, ds0)))
    for m in R.ADJ_M:
        A, gA0 = R._rnd([m, 1], m), R._rnd([m, 2], m)
        for acc in (0, 1):
            total.add('adj_bwd', R.judge_adj_bwd(A, 0.3, gA0, acc, R.twin_adj_bwd(A, 0.3, gA0, acc)))
    print('REG twins: %s' % total.line())
    assert all(e <= 1.0 for k, e in total.items() if not k.startswith('logf'))


def test_bwd_prep_restatement():
    """coef, dao and Gs against the float64 formulas: c_l = d_reg[0] / (2 numel keep), c_e = d_reg[1] / rows, dao = d_ao - 2 c_l I,
    Gs = 4 c_l G; keep = 0 switches the link gradient off."""
    B, C = 3, 7
    G, d_ao = R._rnd(1, B * C * C), R._rnd(2, B * C * C)
    coef, dao, Gs = R.bwd_prep((0.7, -1.3), 2.5, 96.0, 12.0, d_ao, G, B, C)
    cl, ce = float(np.float32(0.7)) / (2 * 96.0 * 2.5), float(np.float32(-1.3)) / 12.0
    assert abs(coef[0] - cl) <= R.U * abs(cl) and abs(coef[1] - ce) <= R.U * abs(ce)
    want = d_ao.reshape(B, C, C).astype(np.float64) - 2 * cl * np.eye(C)
    assert np.abs(dao - want).max() <= 2 * R.U * np.abs(want).max() and np.allclose(Gs, 4 * cl * G.reshape(B, C, C), rtol=3 * R.U, atol=0)
    coef, dao, Gs = R.bwd_prep((0.7, 0.9), 0.0, 96.0, 12.0, None, G, B, C)
    assert coef[0] == 0 and not dao.any() and not Gs.any() and coef[1] == np.float32(float(np.float32(0.9)) / 12.0)


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_mutants_are_rejected(mutant):
    cs = R.forward_cases()
    shown = 0
    if mutant in ('eps_missing', 'sumsq_reads_cap', 'vector_tail_dropped', 'sqrt_negative'):
        for name, c in cs.items():
            can = {'eps_missing': bool((c.S == 0).any()),                                  # 0 * log(0)
                   'sumsq_reads_cap': c.rowptr is not None and c.A is not None,
                   'vector_tail_dropped': c.rowptr is None and c.a_off == 0 and c.A.size % 4 != 0 and R.forward(c).T > 0,
                   'sqrt_negative': R.forward(c).T < 0}[mutant]
            bad = not all(e <= 1.0 for e in _forward_excess(c, mutant).values())
            assert bad == can, name
            shown += can
    if mutant in ('eps_missing', 'no_ratio_term'):
        for rows in R.ROW_CASES_BWD:
            if rows.n:
                S, ds0 = R.rows_matrix(rows.n, rows.C), R._rnd([rows.n, rows.C, 1], rows.n, rows.C)
                assert R.judge_entropy_bwd(S, -0.37, ds0, R.twin_entropy_bwd(S, -0.37, ds0, mutant)) > 1.0, rows
                shown += 1
    if mutant == 'diag_wrong_element':
        for B, C in R.PREP_BC:
            G, d_ao = R._rnd([B, C], B * C * C), R._rnd([C, B], B * C * C)
            same = all(np.array_equal(a, b) for a, b in zip(R.bwd_prep((0.7, -1.3), 2.5, 96.0, 12.0, d_ao, G, B, C),
                                                            R.bwd_prep((0.7, -1.3), 2.5, 96.0, 12.0, d_ao, G, B, C, mutant)))
            assert same == (B == 1), (B, C)                 # a single graph has no row index beyond C
            shown += not same
    if mutant == 'accumulate_ignored':
        for m in R.ADJ_M:
            A, gA0 = R._rnd([m, 1], m), R._rnd([m, 2], m)
            assert R.judge_adj_bwd(A, 0.3, gA0, 1, R.twin_adj_bwd(A, 0.3, gA0, 1, mutant)) > 1.0
            shown += 1
    assert shown
