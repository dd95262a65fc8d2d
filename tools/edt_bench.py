#!/usr/bin/env python
"""The distance-transform stage on one 3584 x 3584 tile (nuclei.distance_transform / expand_labels / split_touching, csrc/edt.hip):
  edt_tissue  distance_transform(foreground of the synthetic tissue tile, return_nearest=True): sites = background, dense
  expand      expand_labels(the tile's instance mask, 4): sites = nuclei, the search bounded by the distance
  split       split_touching(foreground, 3): one unbounded and one bounded transform, three labelling calls, torch glue
  edt_sparse  distance_transform of an image with ONE site per 512 x 512 block (sites='nonzero', unbounded): the stated bad case, the
              search window of a pixel is as wide as the distance to its nearest site
Per case: event-timed median ms per call; for the two plain transforms the compulsory traffic (image read once, dist2 and nearest
written once) against the HBM bound and scipy.ndimage.distance_transform_edt on the host on the same image.

    python tools/edt_bench.py [--iters 20] [--no-cpu] [--out profiles/edt_bench.json]

The split per launch comes from a kernel trace of a few calls, taken in a run of its own and folded into the record afterwards:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o edt_tissue -- python tools/edt_bench.py --trace-case edt_tissue
    python tools/edt_bench.py --parse-trace DIR/.../edt_tissue_kernel_trace.csv --trace-case edt_tissue --out profiles/edt_bench.json"""
import argparse
import collections
import csv
import functools
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import nuclei  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak (spec)
TRACE_CALLS = 5
CASES = ('edt_tissue', 'expand', 'split', 'edt_sparse')


@functools.lru_cache(maxsize=None)
def tissue_labels(size, count):
    return nuclei.synthetic_tissue(size, size, count, seed=0)[0]


def make_case(name, size, count, dev):
    """(callable, host image the plain transform sees or None, its ``sites`` mode, the tensor on the GPU)"""
    if name == 'edt_sparse':
        img = np.zeros((size, size), bool)
        img[256::512, 256::512] = True
        t = torch.from_numpy(img).to(dev)
        return (lambda: nuclei.distance_transform(t, sites='nonzero', return_nearest=True)), img, 'nonzero', t
    labels = tissue_labels(size, count)
    if name == 'edt_tissue':
        img = labels > 0
        t = torch.from_numpy(img).to(dev)
        return (lambda: nuclei.distance_transform(t, return_nearest=True)), img, 'zero', t
    if name == 'expand':
        t = torch.from_numpy(labels).to(dev)
        return (lambda: nuclei.expand_labels(t, 4)), None, None, t
    t = torch.from_numpy(labels > 0).to(dev)
    return (lambda: nuclei.split_touching(t, 3)), None, None, t


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def parse_trace(path):
    """Mean microseconds per launch and launches per call of every kernel in a rocprofv3 kernel_trace.csv (TRACE_CALLS calls)."""
    dur = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r'k_(?:edt|label)_\w+', r['Kernel_Name'])
            name = m.group(0) if m else 'torch: ' + re.sub(r'<.*', '', r['Kernel_Name'])[-60:]
            dur[name].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3)
    out = {k: dict(mean_us=round(float(np.mean(v)), 2), per_call=round(len(v) / float(TRACE_CALLS), 2),
                   us_per_call=round(float(np.sum(v)) / TRACE_CALLS, 2)) for k, v in dur.items()}
    total = sum(v['us_per_call'] for v in out.values())
    return dict(kernels=out, sum_us_per_call=round(total, 2), edt_us_per_call=round(sum(v['us_per_call'] for k, v in out.items()
                                                                                        if k.startswith('k_edt_')), 2),
                note='rocprofv3 --kernel-trace --stats, %d calls' % TRACE_CALLS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--trace-case', choices=CASES, default=None)
    ap.add_argument('--parse-trace', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.parse_trace:
        rec = json.load(open(a.out))
        rec['cases'][a.trace_case]['rocprofv3_kernel_trace'] = parse_trace(a.parse_trace)
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps(rec['cases'][a.trace_case]['rocprofv3_kernel_trace']))
        return
    dev = torch.device('cuda:0')
    if a.trace_case:
        fn = make_case(a.trace_case, a.size, a.nuclei, dev)[0]
        for _ in range(TRACE_CALLS):
            fn()
        torch.cuda.synchronize()
        return
    rec = dict(tile='%dx%d' % (a.size, a.size), iters=a.iters, device=torch.cuda.get_device_name(0), cases={})
    for name in CASES:
        fn, img, sites, t = make_case(name, a.size, a.nuclei, dev)
        out = fn()
        ms = median_ms(fn, a.iters)
        r = dict(ms_per_call=round(ms, 4), ns_per_pixel=round(ms * 1e6 / (a.size * a.size), 4))
        if img is not None:
            d2, near = out
            nbytes = img.nbytes + d2.numel() * 4 + near.numel() * 4
            d2only = median_ms(lambda: nuclei.distance_transform(t, sites=sites), a.iters)
            fin = d2[d2 < nuclei.EDT_INF]
            r.update(site_fraction=round(float(img.mean() if sites == 'nonzero' else 1 - img.mean()), 6),
                     max_dist2=int(fin.max()), mean_distance=round(float(fin.double().sqrt().mean()), 3),
                     ms_per_call_dist2_only=round(d2only, 4), compulsory_bytes=nbytes,
                     hbm_bound_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 4), hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4))
            if not a.no_cpu:
                from scipy import ndimage
                t0 = time.perf_counter()
                want = ndimage.distance_transform_edt(img if sites == 'zero' else ~img)
                r['scipy_distance_transform_edt_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                r['equals_scipy'] = bool(np.array_equal(np.sqrt(d2.cpu().numpy().astype(np.float64)), want))
        elif name == 'split':
            r.update(instances=out[1], components_of_the_mask=nuclei.label_instances(t)[1])
        rec['cases'][name] = r
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
