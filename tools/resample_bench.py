#!/usr/bin/env python
"""Resampling (csrc/resample.hip; kernels.KernelSpec.resample_u8 / resample_labels) beside the stock-torch route on the same device:
  gray/area, gray/linear        resize of a size x size uint8 plane to half size ('area') and to double size ('linear')
  bgr/area, bgr/linear          the same for an interleaved [size, size, 3] tile
  labels/majority, /nearest     resize_labels of the int32 labels of ``synthetic_tissue(size, size, nuclei)`` to half and to double size
  torch/...                     the stock route for each: uint8 -> float32, F.interpolate ('area' / 'bilinear' / 'nearest'; the tile
                                permuted to [1, 3, H, W] and back), round, -> uint8 (labels: int32 -> float32 -> int32; 'nearest' also
                                stands beside 'majority', which stock torch cannot do).  It is a route, not an equal: its result
                                depends on float evaluation order and is not compared here.
Every case reports the bytes its call must move -- the source once plus the output once -- and the bytes per second that makes at
the median time.  Device events around ``--batch`` calls in a row, the median, minimum and maximum over ``--repeats`` (>= 20) such
windows after a warm-up; the cases take turns, window by window.  No time is asserted anywhere.

    python tools/resample_bench.py --out profiles/resample_bench.json
The tool itself never touches the GPU: the measurement is a step, a child process under ``timeout -k 10 --step-limit``, and a step
that fails ends the run with its exit status."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(a):
    """Every case on the GPU: prints one JSON object."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import nuclei

    dev = torch.device('cuda:0')
    n = a.size
    half, double = (n // 2, n // 2), (2 * n, 2 * n)
    gen = torch.Generator(device='cpu').manual_seed(0)
    gray = torch.randint(0, 256, (n, n), dtype=torch.uint8, generator=gen).to(dev)
    bgr = torch.randint(0, 256, (n, n, 3), dtype=torch.uint8, generator=gen).to(dev)
    labels = torch.from_numpy(np.asarray(nuclei.synthetic_tissue(n, n, a.nuclei)[0], np.int32)).to(dev)

    def stock_u8(img, size, mode):
        x = img.to(torch.float32)
        x = x[None, None] if img.dim() == 2 else x.permute(2, 0, 1)[None]
        kw = dict(align_corners=False) if mode == 'bilinear' else {}
        y = F.interpolate(x, size=size, mode=mode, **kw).round_().to(torch.uint8)
        return y[0, 0] if img.dim() == 2 else y[0].permute(1, 2, 0).contiguous()

    def stock_labels(lab, size):
        return F.interpolate(lab.to(torch.float32)[None, None], size=size, mode='nearest')[0, 0].to(torch.int32)

    def moved(src, size):
        return src.numel() * src.element_size() + size[0] * size[1] * src.element_size() * (src.shape[2] if src.dim() == 3 else 1)

    cases = [('gray/area', lambda: nuclei.resize(gray, half, 'area'), moved(gray, half)),
             ('torch/gray/area', lambda: stock_u8(gray, half, 'area'), moved(gray, half)),
             ('gray/linear', lambda: nuclei.resize(gray, double), moved(gray, double)),
             ('torch/gray/linear', lambda: stock_u8(gray, double, 'bilinear'), moved(gray, double)),
             ('bgr/area', lambda: nuclei.resize(bgr, half, 'area'), moved(bgr, half)),
             ('torch/bgr/area', lambda: stock_u8(bgr, half, 'area'), moved(bgr, half)),
             ('bgr/linear', lambda: nuclei.resize(bgr, double), moved(bgr, double)),
             ('torch/bgr/linear', lambda: stock_u8(bgr, double, 'bilinear'), moved(bgr, double)),
             ('labels/majority', lambda: nuclei.resize_labels(labels, half, 'majority'), moved(labels, half)),
             ('torch/labels/nearest_down', lambda: stock_labels(labels, half), moved(labels, half)),
             ('labels/nearest', lambda: nuclei.resize_labels(labels, double), moved(labels, double)),
             ('torch/labels/nearest', lambda: stock_labels(labels, double), moved(labels, double))]
    for _, fn, _ in cases:                                                       # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for window in range(a.repeats):
        for name, fn, _ in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.batch):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / a.batch)
    rec = dict(device=torch.cuda.get_device_name(0), cases={})
    for name, _, nbytes in cases:
        ts = times[name]
        med = float(np.median(ts))
        rec['cases'][name] = dict(ms_median=round(med, 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), bytes_moved=nbytes,
                                  gb_per_s=round(nbytes / med / 1e6, 1))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=4000)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--step', action='store_true', help='run the measurement on the GPU (what the tool starts)')
    ap.add_argument('--step-limit', type=int, default=300, help='seconds the step may take')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    if a.step:
        step(a)
        return
    rec = dict(plane='%dx%d' % (a.size, a.size), nuclei=a.nuclei, repeats=a.repeats, batch=a.batch)
    cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', '--size', str(a.size),
           '--nuclei', str(a.nuclei), '--repeats', str(a.repeats), '--batch', str(a.batch)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)   # the GPU step under its own time limit
    if done.returncode != 0:
        sys.stdout.write(done.stdout)
        print('resample_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
