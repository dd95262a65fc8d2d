"""Nucleus features on the GPU (csrc/nuclei.hip through cgc_net_amd.nuclei) against the float64 restatement tests/nuclei_ref.py."""
import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import network, nuclei
from cgc_net_amd.data import Batch

import nuclei_ref as ref
from nuclei_cases import _gpu, check_against_reference

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('size,count,seed', [(512, 120, 0), (512, 120, 1), (512, 160, 2), (2048, 1800, 0), (2048, 1800, 1),
                                             (3584, 8000, 0)])
def test_synthetic_tiles_match_the_restatement(size, count, seed):
    labels, gray = nuclei.synthetic_tissue(size, size, count, seed)
    _, _, k, info = check_against_reference(labels, gray)
    assert k.size > 0.5 * count and (info[:, 3] == 0).any()


def test_large_nucleus_split_label_and_edges():
    labels, gray = nuclei.synthetic_tissue(512, 512, 100, seed=7)
    yy, xx = np.mgrid[0:512, 0:512]
    labels[((xx - 300) / 45.0) ** 2 + ((yy - 250) / 30.0) ** 2 <= 1] = 99991     # crop ~ 92 x 62 > the LDS limit
    labels[100:110, 40:52] = 99993                                                # one label in two pieces
    labels[130:138, 60:66] = 99993
    f, c, k, info = check_against_reference(labels, gray)
    big = int(np.nonzero(k == 99991)[0][0])
    assert info[big, 3] == 1 and (info[:, 3] == 1).sum() >= 1
    two = int(np.nonzero(k == 99993)[0][0])
    assert np.allclose(c[two], [(10 * 12 * 104.5 + 8 * 6 * 133.5) / 168, (120 * 45.5 + 48 * 62.5) / 168])
    for edge in (labels[0], labels[-1], labels[:, 0], labels[:, -1]):
        assert np.isin(edge[edge > 0], k).any()


def test_bitwise_reproducible():
    labels, gray = nuclei.synthetic_tissue(1024, 1024, 500, seed=4)
    labels[((np.mgrid[0:1024, 0:1024][1] - 500) / 50.0) ** 2 + ((np.mgrid[0:1024, 0:1024][0] - 500) / 40.0) ** 2 <= 1] = 77777
    a = _gpu(labels, gray)
    b = _gpu(labels, gray)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_dtypes_empty_and_refusals():
    labels, gray = nuclei.synthetic_tissue(256, 256, 40, seed=5)
    a = _gpu(labels, gray)
    b = _gpu(labels.astype(np.int64), gray)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    f, c, k = nuclei.nucleus_features(torch.zeros(64, 64, dtype=torch.int32, device=DEV), torch.zeros(64, 64, dtype=torch.uint8, device=DEV))
    assert f.shape == (0, 16) and c.shape == (0, 2) and k.numel() == 0
    tiny = torch.zeros(64, 64, dtype=torch.int32, device=DEV)
    tiny[3:5, 3:5] = 8                                                       # 4 px: removed -> empty
    assert nuclei.nucleus_features(tiny, torch.zeros_like(tiny, dtype=torch.uint8))[0].shape == (0, 16)
    neg = torch.from_numpy(labels).to(DEV)
    neg[10, 10] = -3
    with pytest.raises(ValueError):
        nuclei.nucleus_features(neg, torch.from_numpy(gray).to(DEV))


def test_bgr_to_gray_bit_exact():
    rng = np.random.RandomState(0)
    bgr = rng.randint(0, 256, size=(300, 517, 3)).astype(np.uint8)
    g = nuclei.bgr_to_gray(torch.from_numpy(bgr).to(DEV)).cpu().numpy()
    assert np.array_equal(g, ref.bgr_to_gray(bgr))


def test_tile_to_training_step():
    items = []
    for i in range(4):
        labels, gray = nuclei.synthetic_tissue(512, 512, 150, seed=20 + i)
        f, c, _ = nuclei.nucleus_features(torch.from_numpy(labels).to(DEV), torch.from_numpy(gray).to(DEV))
        items.append(nuclei.graph_item(f, c, i % 3))
    x = torch.cat([d.x for d in items])
    mean, std = x.mean(0), x.std(0) + 1e-3
    batch = Batch.from_data_list(items, device=DEV, knn=(100, 8), mean=mean, std=std)
    torch.manual_seed(0)
    model = network.SoftPoolingGcnEncoder(300, 18, 20, 20, True, True, 20, 3, 0.1, [50], concat=True, load_data_sparse=True,
                                          norm_adj=True, jk=True, drop_out=0.).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    model.train()
    logits, loss = model(batch)
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert logits.shape == (4, 3) and torch.isfinite(loss).item()
    assert all(torch.isfinite(p).all().item() for p in model.parameters())
