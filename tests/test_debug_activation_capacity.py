"""Host only: Context.debug_activation allocates, for every `what` and every geometry the GPU tests run, at least the floats
paac_debug_activation copies -- the library's own count (paac_debug_activation_size) and the oracle's layer shapes agree
with the Python size formula.  (The copy itself refuses an `out` smaller than the activation: a C-side capacity guard.)"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHATS = (1, 2, 3, 4, 11, 12, 13, 14, 21, 22, 23, 24)


def _size_fn(path):
    fn = ctypes.CDLL(path).paac_debug_activation_size
    fn.restype = ctypes.c_int64
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return fn


def _expected(convs, fc, what, batch, arch_name):
    from oracle import network as onet
    dims, _, fc_o = onet.layer_dims(arch_name)
    assert fc_o == fc and [(d["cout"], d["kh"], d["stride"]) for d in dims] == [tuple(c) for c in convs]
    base = what - 20 if what > 20 else (what - 10 if what > 10 else what)
    if base == 4:
        return batch * fc
    if base <= len(dims):
        d = dims[base - 1]
        return batch * d["oh"] * d["ow"] * d["cout"]
    return None


def _check(fn, arch_id, convs, fc, arch_name):
    from paac_amd import hip_ops
    for what in WHATS:
        for batch in (1, 17, 600):
            want = _expected(convs, fc, what, batch, arch_name)
            assert hip_ops.activation_size(convs, fc, what, batch) == want, (convs, fc, what, batch)
            assert fn(arch_id, what, batch) == (-1 if want is None else want), (convs, fc, what, batch)


def test_stock_geometries():
    from paac_amd import _lib, build, hip_ops
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    fn = _size_fn(_lib.LIB_PATH)
    for arch_id, name in ((_lib.ARCH_NATURE, "NATURE"), (_lib.ARCH_NIPS, "NIPS")):
        _check(fn, arch_id, *hip_ops.STOCK_GEOMETRY[arch_id], name)


def test_user_geometries_the_gpu_tests_run():
    sys.path.insert(0, ROOT)
    import __graft_entry__
    from oracle import network as onet
    from paac_amd import _lib, build, hip_ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_user_arch_geometries_gpu import GEOMETRIES
    assert {spec for _, spec in GEOMETRIES} <= set(__graft_entry__.USER_ARCHS)     # build() makes every library they load
    largest = 0
    try:
        for spec in __graft_entry__.USER_ARCHS:
            convs, fc = build.parse_user_arch(spec)
            onet.ARCHS["_CAPACITY"] = (convs, fc)
            path = build.build_user_arch(convs, fc)
            fn = _size_fn(path)
            _check(fn, _lib.ARCH_USER, convs, fc, "_CAPACITY")
            _check(fn, _lib.ARCH_NATURE, *hip_ops.STOCK_GEOMETRY[_lib.ARCH_NATURE], "NATURE")  # Nature rides along
            largest = max(largest, max(hip_ops.activation_size(convs, fc, w, 1) or 0 for w in WHATS))
    finally:
        onet.ARCHS.pop("_CAPACITY", None)
    assert largest > 20 * 20 * 64          # the matrix holds activations above the stock trunks' largest one


def test_activation_size_rejects_what_the_geometry_lacks():
    from paac_amd import hip_ops
    assert hip_ops.activation_size([(16, 8, 4), (32, 4, 2)], 256, 3, 4) is None
    assert hip_ops.activation_size([(16, 8, 4), (32, 4, 2)], 256, 13, 4) is None
    assert hip_ops.activation_size([(16, 8, 4), (32, 4, 2)], 256, 5, 4) is None
    assert hip_ops.activation_size([(16, 4, 2), (32, 1, 1), (48, 5, 5)], 1024, 21, 2) == 2 * 41 * 41 * 16
