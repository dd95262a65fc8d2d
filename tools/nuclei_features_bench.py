#!/usr/bin/env python
"""Nucleus features of one 3584 x 3584 synthetic tile (~8000 nuclei): event-timed ms per tile (warm-up, median), nuclei/s, the label
pass's share of the HBM bound, and the float64 restatement's single-process CPU time on the same tile (tests/nuclei_ref.py).

    python tools/nuclei_features_bench.py [--iters 20] [--no-cpu] [--out profiles/nuclei_features_bench.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import kernels, nuclei  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak (spec)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8000)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    labels, gray = nuclei.synthetic_tissue(a.size, a.size, a.nuclei, seed=0)
    L, G = torch.from_numpy(labels).to(dev), torch.from_numpy(gray).to(dev)
    f, _, kept = nuclei.nucleus_features(L, G)
    n = int(kept.numel())
    tile_ms = median_ms(lambda: nuclei.nucleus_features(L, G), a.iters)

    K = kernels.get()                                    # the label pass (+ init + compaction) alone, no host read
    max_label = int(labels.max())
    ws = torch.empty(int(K.lib.cgc_nuclei_ws_bytes(max_label)), dtype=torch.uint8, device=dev)
    kept_buf = torch.empty(max_label, dtype=torch.int32, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)

    def label_pass():
        rc = K.lib.cgc_nuclei_label_pass(L.data_ptr(), a.size, a.size, max_label, 10, ws.data_ptr(), kept_buf.data_ptr(),
                                         meta.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    pass_ms = median_ms(label_pass, a.iters)
    label_bytes = labels.nbytes
    rec = dict(tile='%dx%d' % (a.size, a.size), nuclei_painted=a.nuclei, rows=n, max_label=max_label,
               ms_per_tile=round(tile_ms, 3), nuclei_per_s=round(n / (tile_ms * 1e-3)),
               label_pass_ms=round(pass_ms, 4), label_pass_bytes=label_bytes,
               label_pass_hbm_fraction=round(label_bytes / (pass_ms * 1e-3) / HBM_BYTES_PER_S, 4),
               big_crops=int((nuclei.nucleus_features(L, G, return_info=True)[3][:, 3] == 1).sum()),
               device=torch.cuda.get_device_name(0))
    if not a.no_cpu:
        import nuclei_ref
        t0 = time.process_time()
        rf, _, _, _ = nuclei_ref.nucleus_features(labels, gray)
        rec['cpu_restatement_s'] = round(time.process_time() - t0, 2)
        rec['cpu_rows_equal'] = bool(rf.shape[0] == n)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
