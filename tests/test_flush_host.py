"""The batched PUT's surface, checked without a GPU: the prototype in
include/bloomhip.h, the exported symbol, the Python binding's signature, the
build's lists of kernel sources, the geometry mirrored in Python, and the
argument checks bloomhip_flush_batch makes before its first HIP call."""
import ctypes
import inspect
import os
import re

import numpy as np

import bloomhip as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs265-lsm-tree_amd", "csrc")

PROTOTYPE = """
int bloomhip_flush_batch(const void *ops, size_t n, int ops_on_device, int drop_tombstones,
                         void *out_entries, size_t *n_out, int out_on_device,
                         bloomhip_filter *f, int device, void *stream);
"""


def _squash(text):
    return re.sub(r"\s+", " ", text).strip()


def _header():
    with open(os.path.join(ROOT, "include", "bloomhip.h")) as fh:
        return fh.read()


def test_header_declares_exactly_the_prototype():
    decls = re.findall(r"^int bloomhip_flush_batch\([^;]*;", _header(), re.M)
    assert len(decls) == 1
    assert _squash(decls[0]) == _squash(PROTOTYPE)


def test_abi_version_and_profiler_slots_unchanged():
    text = _header()
    assert re.search(r"^#define BLOOMHIP_ABI_VERSION 1$", text, re.M)
    assert re.search(r"^#define BLOOMHIP_PROF_SLOTS 13$", text, re.M)
    assert bh.PROF_SLOTS == 13


def test_symbol_exported_and_listed():
    assert hasattr(bh.lib(), "bloomhip_flush_batch")  # a dlsym of the loaded library
    assert "bloomhip_flush_batch" in bh.EXPORTED_SYMBOLS


def test_python_signature():
    sig = inspect.signature(bh.flush_batch)
    assert list(sig.parameters) == ["ops", "drop_tombstones", "filter", "device", "out", "stream"]
    defaults = {k: p.default for k, p in sig.parameters.items()
                if p.default is not inspect.Parameter.empty}
    assert defaults == {"drop_tombstones": False, "filter": None, "device": 0, "out": None,
                        "stream": None}


def _make_var(name):
    with open(os.path.join(CSRC, "Makefile")) as fh:
        text = fh.read().replace("\\\n", " ")
    m = re.search(rf"^{name}\s*:?=\s*(.*)$", text, re.M)
    assert m, name
    return m.group(1).split()


def test_flush_unit_is_built_and_in_the_digest():
    assert "bloom_flush" in _make_var("KERNEL_UNITS")
    srcs = _make_var("KERNEL_SRCS")
    for name in ("bloom_flush.hip", "bloom_flush.h"):
        assert os.path.exists(os.path.join(CSRC, name))
        assert name in srcs, name
    assert "bloom_flush.h" in _make_var("HDRS")


def test_python_constants_equal_the_headers():
    with open(os.path.join(CSRC, "bloom_flush.h")) as fh:
        text = fh.read()

    def const(kind, name):
        return int(re.search(rf"constexpr {kind} {name} = (\d+);", text).group(1))

    tile, cap = const("uint32_t", "kFlushTile"), const("uint32_t", "kFlushBlockCap")
    chunk = const("uint32_t", "kFlushScanChunk")
    assert (bh.FLUSH_TILE, bh.FLUSH_BLOCK_CAP, bh.FLUSH_SCAN_CHUNK) == (tile, cap, chunk)
    ipt = const("int", "kFlushIpt")
    assert tile == 64 * ipt * const("int", "kFlushTileWaves")
    assert cap == 64 * ipt * const("int", "kFlushBlockWaves")


# --- the argument checks, made before any HIP call: the buffers below are
# never dereferenced (every call is refused, or has n == 0)
def _call(ops, n, ops_dev, out, n_out, out_dev, f=None, device=0):
    return bh.lib().bloomhip_flush_batch(ops, n, ops_dev, 0, out, n_out, out_dev, f, device, None)


def _buffers():
    ops = np.zeros((4, 2), dtype=np.int32)
    out = np.zeros((4, 2), dtype=np.int32)
    assert ops.ctypes.data % 8 == 0 and out.ctypes.data % 8 == 0
    return ops, out, ctypes.c_size_t(77)


def test_einval_without_n_out():
    ops, out, _ = _buffers()
    assert _call(ops.ctypes.data, 4, 0, out.ctypes.data, None, 0) == bh.EINVAL
    assert _call(None, 0, 0, None, None, 0) == bh.EINVAL


def test_einval_for_null_buffers_with_ops():
    ops, out, n_out = _buffers()
    assert _call(None, 4, 0, out.ctypes.data, ctypes.byref(n_out), 0) == bh.EINVAL
    assert _call(ops.ctypes.data, 4, 0, None, ctypes.byref(n_out), 0) == bh.EINVAL
    assert n_out.value == 77


def test_einval_for_misaligned_buffers():
    ops, out, n_out = _buffers()
    o, d = ops.ctypes.data, out.ctypes.data
    # host buffers: 4 bytes
    for off in (1, 2, 3):
        assert _call(o + off, 1, 0, d, ctypes.byref(n_out), 0) == bh.EINVAL
        assert _call(o, 1, 0, d + off, ctypes.byref(n_out), 0) == bh.EINVAL
    # device buffers: 8 bytes (the addresses are only looked at)
    assert _call(o + 4, 1, 1, d, ctypes.byref(n_out), 0) == bh.EINVAL
    assert _call(o, 1, 0, d + 4, ctypes.byref(n_out), 1) == bh.EINVAL
    assert n_out.value == 77


def test_erange_at_the_compaction_limit():
    ops, out, n_out = _buffers()
    for n in (2**32 - 1, 2**32, 2**40):
        assert _call(ops.ctypes.data, n, 0, out.ctypes.data, ctypes.byref(n_out), 0) == bh.ERANGE
    # the checks before it come first
    assert _call(ops.ctypes.data + 1, 2**32 - 1, 0, out.ctypes.data, ctypes.byref(n_out), 0) == bh.EINVAL
    assert n_out.value == 77


def test_no_ops_up_to_the_first_device_call():
    _, _, n_out = _buffers()
    rc = _call(None, 0, 0, None, ctypes.byref(n_out), 0)
    if bh.device_count() == 0:
        assert rc == bh.ENODEV  # the device count is the first HIP call
        assert n_out.value == 77
    else:
        assert rc == bh.OK and n_out.value == 0
        assert _call(None, 0, 0, None, ctypes.byref(n_out), 0, device=10**6) == bh.EINVAL
