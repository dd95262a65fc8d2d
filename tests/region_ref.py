"""A numpy restatement of the region statistics (csrc/region.hip; kernels.KernelSpec.region_statistics, region_histogram,
region_quantiles), written from the definition: np.bincount and np.add.at in int64, a sort-based quantile, positions by
np.flatnonzero(...)[0].  A plain module: no pytest hooks, no fixtures.  tests/test_region_ref_cpu.py pins it against a per-label
double loop, scipy.ndimage and cases written out by hand."""
import numpy as np

MAX_QUANTILES = 8


def counted(labels, within=None):
    """The pixels that are counted somewhere, flattened: all of them, or those where ``within`` is non-zero."""
    labels = np.asarray(labels)
    return np.ones(labels.size, bool) if within is None else (np.asarray(within).reshape(-1) != 0)


def refused(labels, max_label):
    """The number of pixels whose label lies outside [0, max_label] (whatever ``within`` says)."""
    lab = np.asarray(labels).astype(np.int64)
    return int(((lab < 0) | (lab > max_label)).sum())


def statistics(labels, values, max_label, within=None):
    """dict(count, sum, sumsq, min, max, argmin, argmax), each [max_label + 1]; count, min, max, argmin, argmax int32, sum and sumsq
    int64 (sumsq is computed for every dtype here: the caller ignores it for int32 values)."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    val = np.asarray(values).astype(np.int64).reshape(-1)
    R = max_label + 1
    on = counted(labels, within) & (lab >= 0) & (lab <= max_label)
    l, v = lab[on], val[on]
    out = dict(count=np.bincount(l, minlength=R).astype(np.int32), sum=np.zeros(R, np.int64), sumsq=np.zeros(R, np.int64),
               min=np.zeros(R, np.int32), max=np.zeros(R, np.int32), argmin=np.full(R, -1, np.int32), argmax=np.full(R, -1, np.int32))
    np.add.at(out['sum'], l, v)
    np.add.at(out['sumsq'], l, v * v)
    for L in np.unique(l):
        sel = on & (lab == L)
        mn, mx = val[sel].min(), val[sel].max()
        out['min'][L], out['max'][L] = mn, mx
        out['argmin'][L] = np.flatnonzero(sel & (val == mn))[0]
        out['argmax'][L] = np.flatnonzero(sel & (val == mx))[0]
    return out


def histogram(labels, values, max_label, within=None):
    """int32 [max_label + 1, 256]: hist[L][v] = the counted pixels of label L with value v."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    val = np.asarray(values).astype(np.int64).reshape(-1)
    assert val.size == 0 or (val.min() >= 0 and val.max() <= 255)
    R = max_label + 1
    on = counted(labels, within) & (lab >= 0) & (lab <= max_label)
    return np.bincount(lab[on] * 256 + val[on], minlength=R * 256).reshape(R, 256).astype(np.int32)


def quantile_of_sorted(v, q10k):
    """v[min(n - 1, floor(n q10k / 10000))] of the sorted values v in Python integers; 0 for n = 0."""
    n = len(v)
    return 0 if n == 0 else int(v[min(n - 1, n * int(q10k) // 10000)])


def quantiles(labels, values, q10k, max_label, within=None):
    """uint8 [max_label + 1, len(q10k)], from the sorted pixels of every region."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    val = np.asarray(values).astype(np.int64).reshape(-1)
    on = counted(labels, within)
    out = np.zeros((max_label + 1, len(q10k)), np.uint8)
    for L in range(max_label + 1):
        v = np.sort(val[on & (lab == L)])
        out[L] = [quantile_of_sorted(v, q) for q in q10k]
    return out


def quantiles_of_histogram(hist, q10k):
    """The same rule on histograms whose bins may be too large to expand: the smallest value whose cumulative count exceeds k, in
    int64 (n < 2^31 and q10k <= 10^4: n q10k < 2^45).  uint8 [R, len(q10k)]."""
    cum = np.asarray(hist).astype(np.int64).reshape(-1, 256).cumsum(axis=1)
    n = cum[:, -1]
    out = np.zeros((cum.shape[0], len(q10k)), np.uint8)
    for j, q in enumerate(q10k):
        k = np.minimum(n - 1, n * int(q) // 10000)
        out[:, j] = np.where(n > 0, (cum > k[:, None]).argmax(axis=1), 0)
    return out


def mean_std(values, labels, max_label, within=None):
    """(mean, std) float64 [max_label + 1] by the two-pass formula over the pixels themselves; 0 for an empty region."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    val = np.asarray(values).astype(np.float64).reshape(-1)
    on = counted(labels, within)
    mean, std = np.zeros(max_label + 1), np.zeros(max_label + 1)
    for L in range(max_label + 1):
        v = val[on & (lab == L)]
        if v.size:
            mean[L] = v.sum() / v.size
            std[L] = np.sqrt(((v - mean[L]) ** 2).sum() / v.size)
    return mean, std
