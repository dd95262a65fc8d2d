"""Host side of the DiffPool regularisers (cgc_level_desc.flags bit 3, include/cgc_hip.h): what the sequencer accepts and how much it
keeps, and the encoder's flag.  Needs the built library (``__graft_entry__.build()``), no GPU."""
import ctypes as C

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels, native, network


def _lib():
    lib = C.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


def _desc(level, flags):
    """The benchmarked C3 configuration (shipped flags: norm_adj + jk), 32 graphs."""
    d = native.LevelDesc()
    d.level, d.fin, d.H, d.E = level, 16 if level == 1 else 20, 20, 20
    d.AH, d.C = (20, {1: 1140, 2: 114}[level]) if level < 3 else (0, 0)
    d.has_bias, d.has_bn, d.act, d.jk, d.renorm, d.renorm_p = 1, 1, 1, 1, 1, 0.4
    for k in range(6):
        d.bn_eps[k], d.bn_momentum[k] = 1e-5, 0.1
    if level == 1:
        d.B, d.n, d.rows_per_graph, d.nmax, d.npad, d.count = 32, 58761, 0, 2000, 2000, 32 * 2000.0
    else:
        R = 1140 if level == 2 else 114
        d.B, d.n, d.rows_per_graph, d.count = 32, 32 * R, R, 32.0 * R
    d.flags = flags
    return d


def test_flag_bit3_only_with_a_pool_block():
    lib = _lib()
    for level in (1, 2):
        assert lib.cgc_level_supported(C.byref(_desc(level, 0)))
        assert lib.cgc_level_supported(C.byref(_desc(level, 8)))
        assert lib.cgc_level_supported(C.byref(_desc(level, 8 | 4)))
        assert lib.cgc_level_supported(C.byref(_desc(level, 8 | 2)))
        assert not lib.cgc_level_supported(C.byref(_desc(level, 16)))
        assert not lib.cgc_level_supported(C.byref(_desc(level, 8 | 16)))
    assert lib.cgc_level_supported(C.byref(_desc(3, 0)))
    assert not lib.cgc_level_supported(C.byref(_desc(3, 8)))


def test_saved_arena_grows_by_the_gram_matrix():
    lib = _lib()
    for level, C_ in ((1, 1140), (2, 114)):
        off, on = _desc(level, 0), _desc(level, 8)
        grow = lib.cgc_level_saved_floats(C.byref(on)) - lib.cgc_level_saved_floats(C.byref(off))
        assert grow >= on.B * C_ * C_, (level, grow)
        assert lib.cgc_level_scratch_floats(C.byref(on)) >= lib.cgc_level_scratch_floats(C.byref(off))


def test_encoder_flag_lists_and_state_dict():
    enc = network.SoftPoolingGcnEncoder(600, 16, 20, 20, True, True, 20, 3, 0.1, [50], diffpool_loss=True)
    assert enc.diffpool_loss is True and enc.link_loss == [] and enc.ent_loss == []
    plain = network.SoftPoolingGcnEncoder(600, 16, 20, 20, True, True, 20, 3, 0.1, [50])
    assert plain.diffpool_loss is False and plain.link_loss == [] and plain.ent_loss == []
    assert list(enc.state_dict().keys()) == list(plain.state_dict().keys())
