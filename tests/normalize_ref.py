"""Reference for stain normalisation (csrc/stain.hip k_od_scan<SCAN_CONC>, k_od_recolor; cgc_net_amd.nuclei.stain_maxima, recolor_matrix,
recolor, normalize_stains): the contracts of kernels.KernelSpec.concentration_histogram / od_recolor, the percentile rule and the matrix
composition restated in numpy int64 and Python integers, with no knowledge of how the kernels work and no code of the package; a float64
Macenko normaliser beside it (np.log, lstsq on the two stain vectors, np.percentile, 255 exp(-C_scaled T)); and the derived bounds
between the two ("Stain normalisation").  The tiles are macenko_ref's.  A plain module: no pytest hooks, no fixtures."""
import functools
import math
from fractions import Fraction

import numpy as np

import macenko_ref

OD_MAX = 5674
BINS = 512                                     # per stain; one level = 1/128 of a natural-log unit
EXP_LEN = 6386
TARGET_STAINS = ((0.5626, 0.7201, 0.4062), (0.2159, 0.8012, 0.5581))
TARGET_MAX = (1.9705, 1.0308)
DEFAULT_STAINS = ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78))

od_lut = macenko_ref.od_lut
od_min_of = macenko_ref.od_min_of
rendered_tile = macenko_ref.rendered_tile


def exp_lut():
    """floor(255 exp(-k / 1024) + 0.5) for k = 0..6385, as int64."""
    return np.array([math.floor(255.0 * math.exp(-k / 1024.0) + 0.5) for k in range(EXP_LEN)], np.int64)


def unit_rows(rows):
    R = np.array(rows, np.float64)
    return R / np.sqrt((R * R).sum(axis=1))[:, None]


def stain_matrix(stains=None):
    """rint(4096 inv(S)) as int64 [3, 3], S the unit-normalised rows; the refusal of the contract asserted."""
    q = np.rint(4096.0 * np.linalg.inv(unit_rows(DEFAULT_STAINS if stains is None else stains))).astype(np.int64)
    assert (np.abs(q).sum(axis=0) * OD_MAX < 2 ** 31 - 2 ** 15).all()
    return q


def od_of(pix, order, lut):
    """int64 [H * W, 3]: (lut[R], lut[G], lut[B]) of every pixel, in raster order."""
    pix = np.asarray(pix)
    rgb = pix[..., ::-1] if order == 0 else pix
    return np.asarray(lut, np.int64)[rgb.astype(np.int64)].reshape(-1, 3)


# ------------------------------------------------------------------ the two kernel contracts
def concentration_histogram(pix, order, lut, od_min, m, within=None):
    """int64 [2 * BINS]: the histogram of b_0, then that of b_1, over the selected pixels."""
    m = np.asarray(m, np.int64)
    assert m.shape == (3, 3) and (np.abs(m).sum(axis=0) * OD_MAX < 2 ** 31 - 2 ** 15).all()
    o = macenko_ref.selected_od(pix, order, lut, od_min, within)
    out = np.zeros(2 * BINS, np.int64)
    for s in range(2):
        C = o @ m[:, s]
        assert np.abs(C).max(initial=0) + 2 ** 14 < 2 ** 31
        b = np.clip((C + 2 ** 14) >> 15, 0, BINS - 1)
        out[BINS * s:BINS * (s + 1)] = np.bincount(b, minlength=BINS)
    return out


def od_recolor(pix, order, lut, a, table):
    """uint8, the shape and channel order of pix."""
    pix = np.asarray(pix)
    a, table = np.asarray(a, np.int64), np.asarray(table, np.int64)
    assert a.shape == (3, 3) and (np.abs(a).sum(axis=0) * OD_MAX < 2 ** 31 - 2 ** 11).all()
    assert table.shape == (EXP_LEN,) and table[0] == 255 and table[-1] == 0 and (np.diff(table) <= 0).all()
    O = od_of(pix, order, lut) @ a                                              # [n, 3]: output channels R, G, B
    assert np.abs(O).max(initial=0) + 2 ** 11 < 2 ** 31
    k = np.clip((O + 2 ** 11) >> 12, 0, EXP_LEN - 1)
    rgb = table[k].astype(np.uint8).reshape(pix.shape)
    return np.ascontiguousarray(rgb[..., ::-1] if order == 0 else rgb)


# ------------------------------------------------------------------ the host rules
def top_bin(bins, alpha):
    """The smallest b with cum(b) >= 1 and 100 cum(b) >= (100 - alpha) n, in exact arithmetic; None for n = 0."""
    a, n = Fraction(alpha), int(sum(int(c) for c in bins))
    cum = np.cumsum([int(c) for c in bins]).tolist()
    ok = [b for b in range(len(cum)) if cum[b] >= 1 and 100 * cum[b] >= (100 - a) * n]
    return min(ok) if n > 0 else None


def stain_maxima(pix, stains=None, order=0, alpha=1.0, beta=0.15, within=None):
    """(maxima as Fractions, bins, n); ValueError as the contract says."""
    counts = concentration_histogram(pix, order, od_lut(), od_min_of(beta), stain_matrix(stains), within)
    n = int(counts[:BINS].sum())
    assert n == int(counts[BINS:].sum())
    if n == 0:
        raise ValueError('no stained pixel')
    bins = tuple(top_bin(counts[BINS * s:BINS * (s + 1)], alpha) for s in range(2))
    if 0 in bins or BINS - 1 in bins:
        raise ValueError('none of a stain, or a saturated histogram')
    return tuple(Fraction(b, 128) for b in bins), bins, n


def recolor_matrix_float(stains, maxima, target_stains=None, target_max=None):
    """A = inv(S)[:, :2] diag(target_max_s / maxima_s) T[:2] in float64."""
    S = unit_rows(stains)
    T = unit_rows(TARGET_STAINS if target_stains is None else target_stains)[:2]
    tm = [float(v) for v in (TARGET_MAX if target_max is None else target_max)]
    mx = [float(v) for v in maxima]
    return np.linalg.inv(S)[:, :2] @ np.diag([tm[0] / mx[0], tm[1] / mx[1]]) @ T


def recolor_matrix(stains, maxima, target_stains=None, target_max=None):
    q = np.rint(4096.0 * recolor_matrix_float(stains, maxima, target_stains, target_max)).astype(np.int64)
    if (np.abs(q).sum(axis=0) * OD_MAX >= 2 ** 31 - 2 ** 11).any():
        raise ValueError('the int32 sum could overflow')
    return q


def normalize(pix, stains=None, order=0, target_stains=None, target_max=None, alpha=1.0, beta=0.15, within=None):
    """The whole integer rule -> (uint8 image, info)."""
    S = macenko_ref.estimate(pix, order, beta, alpha, within)[0] if stains is None else np.array(stains, np.float64)
    maxima, bins, n = stain_maxima(pix, S, order, alpha, beta, within)
    a = recolor_matrix(S, maxima, target_stains, target_max)
    return od_recolor(pix, order, od_lut(), a, exp_lut()), dict(stains=S, maxima=maxima, bins=bins, n=n, matrix=a)


# ------------------------------------------------------------------ the float64 rule
def float_recolor(pix, order, A):
    """255 exp(-(ln(255 / max(v, 1)) A)_d): float64 [n, 3], output channels R, G, B, not clipped."""
    return 255.0 * np.exp(-(macenko_ref.float_od(pix, order) @ np.asarray(A, np.float64)))


def float_normalize(pix, stains, order=0, target_stains=None, target_max=None, alpha=1.0, beta=0.15, within=None):
    """Macenko's normalisation in float64 with given stain vectors (rows haematoxylin, eosin, ...; only the first two are used):
    concentrations by least squares on the two vectors, their np.percentile(., 100 - alpha) over the stained pixels as maxima,
    255 exp(-C_scaled T).  Returns (float64 [n, 3] R, G, B, not clipped and not rounded, dict(C, sel, P))."""
    od = macenko_ref.float_od(pix, order)
    HE = unit_rows(stains)[:2]
    C = np.linalg.lstsq(HE.T, od.T, rcond=None)[0]                              # [2, n]
    sel = (od >= beta).all(axis=1)
    if within is not None:
        sel &= np.asarray(within).reshape(-1) != 0
    P = np.array([np.percentile(C[s][sel], 100.0 - alpha) for s in range(2)])
    T = unit_rows(TARGET_STAINS if target_stains is None else target_stains)[:2]
    tm = np.array(TARGET_MAX if target_max is None else target_max, np.float64)
    return 255.0 * np.exp(-((C * (tm / P)[:, None]).T @ T)), dict(C=C, sel=sel, P=P)


# ------------------------------------------------------------------ the derived bounds
def recolor_bound(pix, order, A):
    """Per pixel and output channel, the most that od_recolor with a = rint(4096 A) may differ from min(float_recolor, 255), in
    levels.  With o_c = lut[v_c] = 1024 L_c + e_c, |e_c| <= 1/2, and a_cd = 4096 A_cd + h_cd, |h_cd| <= 1/2:
        sum_c o_c a_cd - 2^22 sum_c L_c A_cd = 4096 sum_c e_c A_cd + sum_c o_c h_cd,
    so the optical density in 1/1024 is off by at most sum_c |A_cd| / 2 + sum_c o_c / 8192, and k by 1/2 more: delta_d natural-log
    units in all.  exp_lut[k] is 255 exp(-k / 1024) rounded, so the level is off by at most F (exp(delta_d) - 1) + 1/2 with
    F = 255 exp(-O) the unclipped float value; the clamps of k only bring the two sides closer once the float value is cut at 255."""
    A = np.asarray(A, np.float64)
    o = od_of(pix, order, od_lut()).astype(np.float64)
    delta = (0.5 * np.abs(A).sum(axis=0)[None, :] + o.sum(axis=1)[:, None] / 8192.0 + 0.5) / 1024.0
    return float_recolor(pix, order, A) * np.expm1(delta) + 0.5 + 1e-9


def normalize_bound(pix, stains, order=0, target_stains=None, target_max=None, alpha=1.0, beta=0.15, within=None):
    """Per pixel and channel, the most that normalize(pix, stains) may differ from min(float_normalize(pix, stains), 255), in levels,
    with its terms.  Inputs: the tile and the float64 rule's own concentrations and percentiles -- never the integer rule's result.

    1.  gamma_s: a stained pixel's integer concentration C_s / 2^22 against the float one, as in recolor_bound with inv(S) for A:
        (sum_c |inv(S)_cs| / 2 + sum_c o_c / 8192) / 1024, the largest over the stained pixels.
    2.  Half a bin, 1/256: the integer rule reports the centre of the bin.
    3.  rho_s: rounding to bins is monotone, so the bin of the integer rule is that of the order statistic of 0-based rank
        k = ceil((100 - alpha) n / 100) - 1; order statistics move by at most gamma_s when every value does; and numpy's interpolated
        position (n - 1) (100 - alpha) / 100 lies in (k - 1, k + 1): rho_s = sorted[k + 1] - sorted[k - 1] of the float concentrations.
        mu_s = gamma_s + 1/256 + rho_s bounds |b_s / 128 - P_s|.
    4.  With M_s >= P_s - mu_s the scale factors differ by |1 / M_s - 1 / P_s| <= mu_s / (P_s (P_s - mu_s)): the optical density of
        channel d differs by eps_d = sum_s |C_s| t_s |T_sd| mu_s / (P_s (P_s - mu_s)) between the real-number formulas of the two rules.
    5.  delta_d of recolor_bound with |A_cd| <= sum_s |inv(S)_cs| t_s |T_sd| / (P_s - mu_s).
    The level differs by at most F (exp(eps_d + delta_d) - 1) + 1/2, F the unclipped float value."""
    F, f = float_normalize(pix, stains, order, target_stains, target_max, alpha, beta, within)
    C, sel, P = f['C'], f['sel'], f['P']
    S = unit_rows(stains)
    inv = np.linalg.inv(S)
    assert np.abs(inv[:, :2].T @ macenko_ref.float_od(pix, order).T - C).max() < 1e-9, 'the residual row is not orthogonal'
    o = od_of(pix, order, od_lut())
    chosen = (o >= od_min_of(beta)).all(axis=1)
    if within is not None:
        chosen &= np.asarray(within).reshape(-1) != 0
    assert np.array_equal(chosen, sel), 'the two rules select different pixels: the bound does not apply'
    n = int(sel.sum())
    osum = o.sum(axis=1).astype(np.float64)
    T = unit_rows(TARGET_STAINS if target_stains is None else target_stains)[:2]
    tm = np.array(TARGET_MAX if target_max is None else target_max, np.float64)
    k = max(math.ceil((100 - Fraction(alpha)) * n / 100), 1) - 1
    mu, terms = np.zeros(2), []
    for s in range(2):
        gamma = float((0.5 * np.abs(inv[:, s]).sum() + osum[sel].max() / 8192.0) / 1024.0)
        srt = np.sort(C[s][sel])
        rho = float(srt[min(k + 1, n - 1)] - srt[max(k - 1, 0)])
        mu[s] = gamma + 1.0 / 256 + rho + 1e-12
        terms.append(dict(gamma=gamma, half_bin=1.0 / 256, rho=rho, mu=float(mu[s]), P=float(P[s])))
    assert (P - mu > 0).all()
    eps = (np.abs(C) * (tm * mu / (P * (P - mu)))[:, None]).T @ np.abs(T)                          # [n, 3]
    reach = (np.abs(inv[:, :2]) * (tm / (P - mu))[None, :]) @ np.abs(T)                            # [3, 3]: a bound on |A_cd|
    delta = (0.5 * reach.sum(axis=0)[None, :] + osum[:, None] / 8192.0 + 0.5) / 1024.0
    return F * np.expm1(eps + delta) + 0.5 + 1e-9, F, terms


def float_normalized_tile(pix, stains, order=0, **kw):
    """The float64 normaliser's result as an image: cut at 255, rounded to bytes, in the channel order of pix."""
    rgb = np.clip(np.rint(float_normalize(pix, stains, order, **kw)[0]), 0, 255).astype(np.uint8).reshape(np.asarray(pix).shape)
    return np.ascontiguousarray(rgb[..., ::-1] if order == 0 else rgb)


def estimate_shift_bound(U, V, order=0, beta=0.15, alpha=1.0):
    """The most that a stain vector of the float64 Macenko estimate (macenko_ref.float_macenko) may turn between two images of one
    tile, U and V, in degrees, with its terms -- the bound of DESIGN.md, "Stain estimation", for a perturbation of the pixels in place
    of the rounding of a table.  Inputs: the two images' optical densities and the float64 rule's covariance and sorted angles on V --
    never the vectors that are compared.
        B = 2 tau + asin(kappa sin tau) + gamma + rho
    tau: the tilt between the two planes, by Davis-Kahan (Yu, Wang and Samworth 2015) from the two covariances as they are, each over
    its own stained pixels.  kappa: as there.  gamma: a pixel's optical densities differ by e_i = |x_i - z_i| between the images, so
    its direction in a plane by at most asin(e_i / (|proj z_i| - sin tau |z_i| - e_i)).  rho: the stained sets differ in m pixels, so a
    rank in one is within m of the rank in the common set and that within m of the rank in the other; with numpy's interpolation one
    more on either side: the gap of V's sorted angles over 2 m + 1 ranks on either side of the percentile's position (and of its
    mirror image)."""
    xU, zV = macenko_ref.float_od(U, order), macenko_ref.float_od(V, order)
    A, Bs = (xU >= beta).all(axis=1), (zV >= beta).all(axis=1)
    f = macenko_ref.float_macenko(V, order, beta, alpha)[1]
    lam, e1, e2 = f['lam'], f['e1'], f['e2']
    sin_tau = 2.0 * np.linalg.norm(np.cov(xU[A].T) - np.cov(zV[Bs].T), 2) / (lam[1] - lam[0])
    assert sin_tau < 0.5
    tau = math.asin(sin_tau)
    both = A | Bs
    z, e = zV[both], np.sqrt(((xU[both] - zV[both]) ** 2).sum(axis=1))
    znorm = np.sqrt((z * z).sum(axis=1))
    proj = np.sqrt((z @ e1) ** 2 + (z @ e2) ** 2)
    kappa = 1.0 / ((proj / znorm).min() - sin_tau)
    room = proj - sin_tau * znorm - e
    assert (room > e).all()
    gamma = float(np.arcsin(e / room).max())
    m, n = int((A ^ Bs).sum()), int(Bs.sum())
    phi = np.sort(f['phi'])
    rho = 0.0
    for q in (Fraction(alpha) / 100, 1 - Fraction(alpha) / 100):
        p = float((n - 1) * q)
        for p in (p, n - 1 - p):                                                  # ... and its mirror image: e_2 may point the other way
            rho = max(rho, float(phi[min(math.ceil(p) + 2 * m + 1, n - 1)] - phi[max(math.floor(p) - 2 * m - 1, 0)]))
    terms = dict(tau=tau, tilt_of_pixels=math.asin(min(1.0, kappa * sin_tau)), gamma=gamma, rho=rho, flipped=m)
    return math.degrees(2 * tau + terms['tilt_of_pixels'] + gamma + rho + 1e-9), terms


def target_matrix(target_stains=None):
    """The 3 x 3 vectors TARGET_STAINS + residual: the two target rows and their cross product, unit-normalised."""
    T = unit_rows(TARGET_STAINS if target_stains is None else target_stains)[:2]
    return unit_rows(np.stack([T[0], T[1], np.cross(T[0], T[1])]))


@functools.lru_cache(maxsize=None)
def normalized_case(shape, pair):
    """(tile BGR, S of the integer rule, normalised tile, info) with estimated stains -- computed once, never modified."""
    tile, S = macenko_ref.rendered_case(shape, pair)[:2]
    out, info = normalize(tile, S)
    out.setflags(write=False)
    return tile, S, out, info
