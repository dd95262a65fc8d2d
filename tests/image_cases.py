"""Inputs that the GPU tests of the distance-transform and geodesic stages share (tests/test_edt_gpu.py, tests/test_geodesic_gpu.py).
A plain module: no pytest hooks, no fixtures."""
import functools

import numpy as np
import torch

from cgc_net_amd import nuclei

DEV = torch.device('cuda:0')
DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def tissue():
    """(labels int32, gray uint8, within bool), each [300, 300]: touching, clipped and ring nuclei, and a porous domain."""
    labels, gray = nuclei.synthetic_tissue(300, 300, 60)
    within = np.random.RandomState(31).rand(300, 300) < 0.7
    return labels, gray, within


def two_discs():
    """Two discs of radius 10 whose centres are 14 apart: one component that an erosion by 8 splits."""
    yy, xx = np.mgrid[0:48, 0:48]
    return ((yy - 24) ** 2 + (xx - 17) ** 2 <= 100) | ((yy - 24) ** 2 + (xx - 31) ** 2 <= 100)
