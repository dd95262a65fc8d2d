#!/usr/bin/env python
"""Connected-component labelling of one 3584 x 3584 mask (nuclei.label_instances, csrc/label.hip) on two images: the foreground of the
synthetic tissue tile (~8000 nuclei) and uniform noise at density 0.59 with connectivity 1 -- the site-percolation threshold, fractal
clusters that span every tile.  Per image: event-timed median ms per call (warm-up, host read of n included), the compulsory traffic
(image read once + labels written once) against the HBM bound, and scipy.ndimage.label on the host on the same image.

    python tools/label_bench.py [--iters 20] [--no-cpu] [--out profiles/label_instances_bench.json]

The split per launch comes from a kernel trace of a few calls, taken in a run of its own and folded into the record afterwards:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tissue -- python tools/label_bench.py --trace-image tissue
    python tools/label_bench.py --parse-trace DIR/.../tissue_kernel_trace.csv --trace-image tissue --out profiles/label_instances_bench.json"""
import argparse
import collections
import csv
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


def make_image(name, size, count):
    if name == 'tissue':
        return nuclei.synthetic_tissue(size, size, count, seed=0)[0] > 0, 1
    return np.random.RandomState(0).rand(size, size) < 0.59, 1


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
    """Mean microseconds per launch of every k_label_* kernel in a rocprofv3 kernel_trace.csv, warm-up calls included."""
    dur = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r'k_label_\w+', r['Kernel_Name'])
            if m:
                dur[m.group(0)].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3)
    out = {k: round(float(np.mean(v)), 2) for k, v in dur.items()}
    out['launches_per_call'] = len(out)
    out['sum_us'] = round(sum(v for k, v in out.items() if k.startswith('k_label_')), 2)
    out['note'] = 'rocprofv3 --kernel-trace --stats, mean per launch over %d calls' % max(len(v) for v in dur.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--trace-image', choices=['tissue', 'noise'], default=None)
    ap.add_argument('--parse-trace', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.parse_trace:
        rec = json.load(open(a.out))
        rec['images'][a.trace_image]['rocprofv3_kernel_trace_us'] = parse_trace(a.parse_trace)
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps(rec['images'][a.trace_image]['rocprofv3_kernel_trace_us']))
        return
    dev = torch.device('cuda:0')
    if a.trace_image:
        img, conn = make_image(a.trace_image, a.size, a.nuclei)
        t = torch.from_numpy(img).to(dev)
        for _ in range(TRACE_CALLS):
            nuclei.label_instances(t, conn)
        torch.cuda.synchronize()
        return
    rec = dict(tile='%dx%d' % (a.size, a.size), iters=a.iters, device=torch.cuda.get_device_name(0), images={})
    for name in ('tissue', 'noise'):
        img, conn = make_image(name, a.size, a.nuclei)
        t = torch.from_numpy(img).to(dev)
        labels, n = nuclei.label_instances(t, conn)
        ms = median_ms(lambda: nuclei.label_instances(t, conn), a.iters)
        ms_sizes = median_ms(lambda: nuclei.label_instances(t, conn, min_size=10, return_sizes=True), a.iters)
        nbytes = img.nbytes + labels.numel() * 4
        r = dict(what='synthetic_tissue(%d, %d, %d) > 0' % (a.size, a.size, a.nuclei) if name == 'tissue' else 'uniform noise, density 0.59',
                 connectivity=conn, foreground_fraction=round(float(img.mean()), 4), components=n,
                 largest_component_px=int(torch.bincount(labels.flatten())[1:].max()),
                 ms_per_call=round(ms, 4), ms_per_call_min_size_10_with_sizes=round(ms_sizes, 4), compulsory_bytes=nbytes,
                 hbm_bound_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 4), hbm_fraction=round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4))
        if not a.no_cpu:
            from scipy import ndimage
            t0 = time.perf_counter()
            want, wn = ndimage.label(img)
            r['scipy_ndimage_label_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            r['equals_scipy'] = bool(wn == n and np.array_equal(labels.cpu().numpy(), want))
        rec['images'][name] = r
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
