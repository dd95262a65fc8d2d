#!/usr/bin/env python
"""Region hull (csrc/region.hip; kernels.KernelSpec.region_hull) beside the region geometry it stands on, and the two routes of its
second stage on regions of growing height:
  geometry                      region_geometry alone: the number to report against
  hull                          the device side of a hull call: region_geometry, the prefix sum, the spans, the chains and the tables
  hull/stages                   ... the two hull launches alone (spans, chains and tables)
  region_hull                   the public function, with its one host read
  hull_features                 the seven columns per nucleus, with its one host read
  tall/<shape>/<H>/short|wave   the two hull launches on an H x W image that is one region -- ``ones``: every pixel; ``ellipse``: the
                                inscribed ellipse, whose hull has many vertices, in a background that is as tall -- with every region on
                                the one-lane route (tall_rows = H) and with every region on the wave route (tall_rows = 1)
The tissue is ``synthetic_tissue(size, size, nuclei)`` as it comes (sparse ids).  Before anything is timed the two routes are
compared for equality.  Device events around ``--batch`` calls in a row, the median, minimum and maximum over ``--repeats`` (>= 20)
such windows after a warm-up; the cases take turns, window by window.  No time is asserted anywhere.

    python tools/hull_bench.py --out profiles/hull_bench.json
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
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import kernels, nuclei

    dev = torch.device('cuda:0')
    table = kernels.get()
    labels_np, _ = nuclei.synthetic_tissue(a.size, a.size, a.nuclei)
    L = torch.from_numpy(np.asarray(labels_np, np.int32)).to(dev)
    n = int(L.max())
    kept = torch.unique(L)[1:].to(torch.int32)

    def prepared(lab, top):
        (count, _, extents, _, _), meta = table.region_geometry(lab, top)
        assert int(meta) == 0
        ptr = table.region_hull_ptr(count, extents)
        return extents, ptr, int(ptr[-1])

    ext, ptr, S = prepared(L, n)

    def device_side():
        (count, _, extents, _, _), _ = table.region_geometry(L, n)
        return table.region_hull(L, n, extents, table.region_hull_ptr(count, extents), S)

    cases = [('geometry', lambda: table.region_geometry(L, n), a.batch),
             ('hull', device_side, a.batch),
             ('hull/stages', lambda: table.region_hull(L, n, ext, ptr, S), a.batch),
             ('region_hull', lambda: nuclei.region_hull(L, max_label=n), 1),
             ('hull_features', lambda: nuclei.hull_features(L, kept, max_label=n), 1)]
    shapes = {}
    for H in a.heights:
        W = H if H >= 2048 else 256
        yy = torch.arange(H, device=dev, dtype=torch.float64)[:, None] + 0.5
        xx = torch.arange(W, device=dev, dtype=torch.float64)[None, :] + 0.5
        images = {'ones': torch.ones(H, W, dtype=torch.int32, device=dev),
                  'ellipse': (((yy - H / 2) / (H / 2)) ** 2 + ((xx - W / 2) / (W / 2)) ** 2 <= 1).to(torch.int32)}
        for shape, lab in images.items():
            e, p, s = prepared(lab, 1)
            short, wave = table.region_hull(lab, 1, e, p, s, tall_rows=H), table.region_hull(lab, 1, e, p, s, tall_rows=1)
            assert all(torch.equal(x, y) for x, y in zip(short[0], wave[0]))      # the two routes agree before they are timed
            shapes['%s/%d' % (shape, H)] = dict(width=W, vertices=short[0][0].tolist())
            for route, rows in (('short', H), ('wave', 1)):
                cases.append(('tall/%s/%d/%s' % (shape, H, route),
                              lambda lab=lab, e=e, p=p, s=s, rows=rows: table.region_hull(lab, 1, e, p, s, tall_rows=rows), 1))
    for _, fn, _ in cases:                                                       # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for window in range(a.repeats):
        for name, fn, batch in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(batch):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / batch)
    rec = dict(device=torch.cuda.get_device_name(0), tall_rows=table.region_hull_tall_rows, labels_with_pixels=int(kept.numel()) + 1,
               table_rows=n + 1, span_rows=S, one_region=shapes, cases={})
    for name, _, _ in cases:
        ts = times[name]
        rec['cases'][name] = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--nuclei', type=int, default=4000)
    ap.add_argument('--heights', type=int, nargs='+', default=[64, 128, 256, 512, 1024, 4096])
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
           '--nuclei', str(a.nuclei), '--repeats', str(a.repeats), '--batch', str(a.batch), '--heights'] + [str(h) for h in a.heights]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)   # the GPU step under its own time limit
    if done.returncode != 0:
        sys.stdout.write(done.stdout)
        print('hull_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
