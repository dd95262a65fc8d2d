"""Reference for stain estimation (csrc/stain.hip k_od_scan; cgc_net_amd.nuclei.estimate_stains): the contracts of
kernels.KernelSpec.od_moments / angle_histogram and items 1-6 of estimate_stains restated in numpy int64 and Python integers, with no
knowledge of how the kernels work and no code of the package -- the angle bin is the COUNT of the contract, not a search --, a float64
Macenko beside it (np.log, np.cov, eigh, arctan2, np.percentile), the rendered two-stain tiles both are run on, and the derived bound
on the angle between their vectors ("Stain estimation").  A plain module: no pytest hooks, no fixtures."""
import functools
import math
from fractions import Fraction

import numpy as np

OD_MAX = 5674
K = 1024
E_MAX, E_REACH, DIR_MAX = 4096, 7095, 16384
P_MAX = 9829                                   # the stated bound on |p_j|; (5674 * 7095 + 2^11) >> 12 = 9828 is the extreme
# (haematoxylin, eosin) unit OD vectors (R, G, B): the pair of Macenko's reference implementation, and Ruifrok and Johnston's
STAIN_PAIRS = (((0.5626, 0.7201, 0.4062), (0.2159, 0.8012, 0.5581)), ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11)))
TILE_SHAPES = ((48, 64), (96, 80), (200, 160))


def od_lut():
    """floor(1024 ln(255 / max(v, 1)) + 0.5) for v = 0..255, as int64."""
    return np.array([math.floor(1024.0 * math.log(255.0 / max(v, 1)) + 0.5) for v in range(256)], np.int64)


def angle_thetas():
    return [-0.5 * math.pi + k * math.pi / K for k in range(1, K)]


def angle_dirs():
    """(rint(16384 cos t_k), rint(16384 sin t_k)), t_k = -pi/2 + k pi / K, k = 1..K-1, as int64 [K - 1, 2]."""
    return np.array([(np.rint(16384.0 * math.cos(t)), np.rint(16384.0 * math.sin(t))) for t in angle_thetas()]).astype(np.int64)


def od_min_of(beta):
    k = 0
    while Fraction(k, 1024) < Fraction(beta):
        k += 1
    return k


def selected_od(pix, order, lut, od_min, within=None):
    """o int64 [n, 3] (R, G, B) of the selected pixels, in raster order."""
    pix = np.asarray(pix)
    rgb = pix[..., ::-1] if order == 0 else pix
    o = np.asarray(lut, np.int64)[rgb.astype(np.int64)].reshape(-1, 3)
    sel = (o >= od_min).all(axis=1)
    if within is not None:
        sel &= np.asarray(within).reshape(-1) != 0
    return o[sel]


def od_moments(pix, order, lut, od_min, within=None):
    """[n, sR, sG, sB, RR, RG, RB, GG, GB, BB] as Python integers."""
    o = selected_od(pix, order, lut, od_min, within)
    cols = [[int(v) for v in o[:, c]] for c in range(3)]
    out = [len(o)] + [sum(c) for c in cols]
    for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append(sum(a * b for a, b in zip(cols[i], cols[j])))
    return out


def project(o, basis):
    """p int64 [n, 2]: p_j = (sum_c o_c E[j][c] + 2^11) >> 12, with the contract's bounds asserted."""
    E = np.asarray(basis, np.int64)
    assert E.shape == (2, 3) and np.abs(E).max() <= E_MAX and (np.abs(E).sum(axis=1) <= E_REACH).all()
    acc = o @ E.T
    assert np.abs(acc).max(initial=0) <= OD_MAX * E_REACH < 2 ** 26
    p = (acc + 2 ** 11) >> 12
    assert np.abs(p).max(initial=0) <= P_MAX
    return p


def count_bins(p, dirs):
    """b = #{k : c_k p_2 - s_k p_1 >= 0} for every row of p int64 [n, 2] -- the count itself, over all K - 1 directions."""
    d = np.asarray(dirs, np.int64)
    assert d.shape == (K - 1, 2) and np.abs(d).max() <= DIR_MAX
    uniq, inverse = np.unique(p, axis=0, return_inverse=True)
    b = np.zeros(len(uniq), np.int64)
    for i in range(0, len(uniq), 4096):
        u = uniq[i:i + 4096]
        cross = u[:, 1:2] * d[None, :, 0] - u[:, 0:1] * d[None, :, 1]
        assert np.abs(cross).max(initial=0) < 2 ** 31
        b[i:i + 4096] = (cross >= 0).sum(axis=1)
    return b[inverse.reshape(-1)]


def angle_histogram(pix, order, lut, od_min, basis, dirs, within=None):
    """int64 [K + 1]: the K bins, then the skipped counter."""
    p = project(selected_od(pix, order, lut, od_min, within), basis)
    out = np.zeros(K + 1, np.int64)
    binned = p[:, 0] > 0
    out[K] = int((~binned).sum())
    out[:K] = np.bincount(count_bins(p[binned], dirs), minlength=K)
    return out


def plane_of_moments(mom):
    """(n, eigenvalues ascending, e_1, e_2) of item 2; ValueError as the contract says."""
    n, s = int(mom[0]), [int(v) for v in mom[1:4]]
    if n < 2:
        raise ValueError('too few stained pixels')
    rr, rg, rb, gg, gb, bb = [int(v) for v in mom[4:]]
    q = [[rr, rg, rb], [rg, gg, gb], [rb, gb, bb]]
    C = np.array([[float(n * q[i][j] - s[i] * s[j]) for j in range(3)] for i in range(3)], np.float64)
    lam, vec = np.linalg.eigh(C)
    if not (np.isfinite(lam[1]) and lam[1] > 0):
        raise ValueError('one stain only')
    return n, lam, orient(vec[:, 2], vec[:, 1])


def orient(e1, e2):
    e1 = -e1 if e1.sum() < 0 else e1.copy()
    e2 = -e2 if e2[np.argmax(np.abs(e2))] < 0 else e2.copy()
    return e1, e2


def percentile_bins(bins, alpha):
    a, M = Fraction(alpha), int(sum(int(c) for c in bins))
    cum = np.cumsum([int(c) for c in bins]).tolist()
    b_lo = min(b for b in range(K) if cum[b] >= 1 and 100 * cum[b] >= a * M)
    b_hi = min(b for b in range(K) if 100 * cum[b] >= (100 - a) * M)
    return b_lo, b_hi


def stains_of_angles(e1, e2, phi_lo, phi_hi):
    """Rows haematoxylin (the larger R component), eosin, their cross product; all normalised."""
    v = [e1 * math.cos(phi) + e2 * math.sin(phi) for phi in (phi_lo, phi_hi)]
    h, e = (v[0], v[1]) if v[0][0] > v[1][0] else (v[1], v[0])
    S = np.stack([h, e, np.cross(h, e)])
    return S / np.sqrt((S * S).sum(axis=1))[:, None]


def estimate(pix, order=0, beta=0.15, alpha=1.0, within=None, moments=None, counts=None, plane=None):
    """Items 1-6 -> (S float64 [3, 3], info).  ``moments`` / ``counts`` replace the restated reductions by given ones, ``plane`` =
    (eigenvalues, e_1, e_2) the eigen-decomposition."""
    lut, od_min = od_lut(), od_min_of(beta)
    mom = od_moments(pix, order, lut, od_min, within) if moments is None else [int(v) for v in moments]
    n, lam, (e1, e2) = plane_of_moments(mom)
    if plane is not None:
        lam, e1, e2 = plane
    basis = np.rint(4096.0 * np.stack([e1, e2])).astype(np.int64)
    counts = angle_histogram(pix, order, lut, od_min, basis, angle_dirs(), within) if counts is None else [int(c) for c in counts]
    if sum(int(c) for c in counts[:K]) == 0:
        raise ValueError('nothing binned')
    b_lo, b_hi = percentile_bins(counts[:K], alpha)
    S = stains_of_angles(e1, e2, *[-0.5 * math.pi + (b + 0.5) * math.pi / K for b in (b_lo, b_hi)])
    info = dict(n=n, skipped=int(counts[K]), od_min=od_min, bins=(b_lo, b_hi), eigenvalues=tuple(float(v) / (n * (n - 1)) for v in lam))
    return S, info, dict(moments=mom, basis=basis, counts=[int(c) for c in counts], e1=e1, e2=e2)


# ------------------------------------------------------------------ the float64 rule
def float_od(pix, order):
    pix = np.asarray(pix)
    rgb = (pix[..., ::-1] if order == 0 else pix).astype(np.float64).reshape(-1, 3)
    return -np.log(np.maximum(rgb, 1.0) / 255.0)


def float_macenko(pix, order=0, beta=0.15, alpha=1.0, within=None):
    """Macenko in float64 -> (S [3, 3], dict(x, lam, e1, e2, phi))."""
    od = float_od(pix, order)
    sel = (od >= beta).all(axis=1)
    if within is not None:
        sel &= np.asarray(within).reshape(-1) != 0
    x = od[sel]
    lam, vec = np.linalg.eigh(np.cov(x.T))
    e1, e2 = orient(vec[:, 2], vec[:, 1])
    phi = np.arctan2(x @ e2, x @ e1)
    S = stains_of_angles(e1, e2, np.percentile(phi, alpha), np.percentile(phi, 100.0 - alpha))
    return S, dict(x=x, lam=lam, e1=e1, e2=e2, normal=vec[:, 0], phi=phi)


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = float(a @ b / math.sqrt(float(a @ a) * float(b @ b)))
    return math.degrees(math.atan2(math.sqrt(max(0.0, 1.0 - c * c)), c))


def table_rounding():
    """The largest angle between a direction of the table and the boundary it stands for, in radians."""
    d = angle_dirs()
    return max(abs(math.atan2(int(s), int(c)) - t) for (c, s), t in zip(d, angle_thetas()))


def derived_bound(pix, order=0, beta=0.15, alpha=1.0, within=None):
    """The bound of DESIGN.md, "Stain estimation", on the angle between a vector of the integer rule and the same vector of the
    float64 rule, in degrees, with its terms.  Inputs: the tile, the table's rounding on that tile, the float64 rule's own
    covariance and sorted angles, and the smallest |p| of the integer rule -- never the vectors that are compared.
        B = 2 tau + asin(kappa sin tau) + gamma + delta + pi / (2 K) + rho"""
    _, f = float_macenko(pix, order, beta, alpha, within)
    x, lam = f['x'], f['lam']
    lut, od_min = od_lut(), od_min_of(beta)
    o = selected_od(pix, order, lut, od_min, within)
    assert len(o) == len(x), 'the two rules select different pixels: the bound does not apply'
    y = o / 1024.0
    # tau: the tilt of the plane.  Davis-Kahan as in Yu, Wang and Samworth (2015): sin <= 2 |cov y - cov x|_2 / (lam_2 - lam_3)
    delta_cov = np.linalg.norm(np.cov(y.T) - np.cov(x.T), 2)
    sin_tau = 2.0 * delta_cov / (lam[1] - lam[0])
    assert sin_tau < 0.5
    tau = math.asin(sin_tau)
    # kappa: |x| over the length of its projection on the integer rule's plane, from the float plane and tau
    inplane = np.sqrt((x @ f['e1']) ** 2 + (x @ f['e2']) ** 2) / np.sqrt((x * x).sum(axis=1))
    kappa = 1.0 / (inplane.min() - sin_tau)
    # gamma: lut, E and p rounded, per pixel: |p_j - P_j| <= sqrt(3) / 2 + |o|_1 / 8192 + 1 / 2
    _, _, z = estimate(pix, order, beta, alpha, within)
    p = project(o, z['basis']).astype(np.float64)
    eta = math.sqrt(2.0) * (math.sqrt(3.0) / 2 + o.sum(axis=1) / 8192.0 + 0.5)
    norm = np.sqrt((p * p).sum(axis=1))
    assert (norm > 2 * eta).all()
    gamma = float(np.arcsin(eta / (norm - eta)).max())
    # rho: the rank the integer rule reads and numpy's interpolated position lie within one order statistic of each other
    phi, M = np.sort(f['phi']), len(x)
    assert np.abs(phi).max() < 0.5 * math.pi
    rho = 0.0
    for frac in (Fraction(alpha) / 100, 1 - Fraction(alpha) / 100):
        k = max(math.ceil(frac * M), 1) - 1                                   # 0-based rank of the integer rule
        for k in (k, M - 1 - k):                                              # ... and its mirror image: e_2 may point the other way
            rho = max(rho, float(phi[min(k + 1, M - 1)] - phi[max(k - 1, 0)]))
    terms = dict(tau=tau, tilt_of_pixels=math.asin(min(1.0, kappa * sin_tau)), gamma=gamma, delta=table_rounding(),
                 half_bin=math.pi / (2 * K), rho=rho, min_p=float(norm.min()))
    total = 2 * tau + terms['tilt_of_pixels'] + gamma + terms['delta'] + terms['half_bin'] + rho + 1e-9
    return math.degrees(total), terms


# ------------------------------------------------------------------ rendered tiles
@functools.lru_cache(maxsize=None)
def rendered_tile(shape, pair, order=0, seed=0):
    """uint8 [H, W, 3] of two known stains: 30 % near-white background, 10 % pure haematoxylin, 10 % pure eosin, 50 % mixtures with
    random non-negative concentrations; rint(255 exp(-OD)) plus noise of one level.  Computed once, never modified."""
    H, W = shape
    h, e = [np.array(v, np.float64) / math.sqrt(sum(c * c for c in v)) for v in STAIN_PAIRS[pair]]
    rng = np.random.RandomState(100 * pair + seed + H)
    kind = rng.rand(H * W)
    cH, cE = rng.uniform(0.0, 2.0, H * W), rng.uniform(0.0, 2.0, H * W)
    back = kind < 0.3
    cH[back], cE[back] = rng.uniform(0.0, 0.03, int(back.sum())), rng.uniform(0.0, 0.03, int(back.sum()))
    pure_h, pure_e = (kind >= 0.3) & (kind < 0.4), (kind >= 0.4) & (kind < 0.5)
    cE[pure_h] = 0.0
    cH[pure_e] = 0.0
    cH[pure_h] += 0.6
    cE[pure_e] += 0.6
    od = cH[:, None] * h + cE[:, None] * e
    rgb = np.rint(255.0 * np.exp(-od)) + rng.randint(-1, 2, (H * W, 3))
    rgb = np.clip(rgb, 0, 255).astype(np.uint8).reshape(H, W, 3)
    tile = np.ascontiguousarray(rgb[..., ::-1] if order == 0 else rgb)
    tile.setflags(write=False)
    return tile


def true_stains(pair):
    return [np.array(v, np.float64) / math.sqrt(sum(c * c for c in v)) for v in STAIN_PAIRS[pair]]


@functools.lru_cache(maxsize=None)
def rendered_case(shape, pair):
    """(tile BGR, S of the integer rule, info, detail, S of the float64 rule) -- computed once, never modified."""
    tile = rendered_tile(shape, pair)
    S, info, z = estimate(tile)
    return tile, S, info, z, float_macenko(tile)[0]
